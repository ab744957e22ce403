# coding=utf-8
"""Writes tests/golden/asap_cases.npz: the outputs of the reference's OWN asap() and cluster_pool() on the inputs of
tests/asap_cases.py, run through oracle/ref_harness (on the numpy stand-ins for TensorFlow / tf_sparse where those are not
installed; the backend is recorded as ``__backend__``).  asap() runs with exactly the two adapters of
asap_cases.install_adapters (the old gcn signature, [node; cluster] assignment rows) and is otherwise unmodified;
cluster_pool() runs as it is.  A digest of every case's inputs is stored next to the outputs.

The generator refuses inputs on which the selection could hang on the last float32 bit: inside every graph, adjacent sorted
node scores (taken from the float64 mirror, tests/asap_mirror.py) must differ by at least asap_cases.MIN_SCORE_GAP; change
asap_cases.WEIGHT_SEED / BATCH_SEED when it fails.

    python tests/golden/make_asap_golden.py          # regenerate (needs the reference checkout)
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from oracle.ref_harness import load_reference   # noqa: E402
import asap_cases as ac                          # noqa: E402
import asap_mirror as am                         # noqa: E402
from make_pool_golden import inputs_digest       # noqa: E402

OUT = os.path.join(HERE, "asap_cases.npz")


def min_score_gap(g):
    """The smallest distance between adjacent sorted node scores of one graph, over every ASAP configuration."""
    worst = np.inf
    for name, kr, act, weighted, _ in ac.ASAP_CONFIGS:
        w = dict(zip(am.WEIGHT_NAMES, ac.config_weights(g, name)))
        m = am.asap_mirror(g["x"], g["ei"], g["w"] if weighted else None, g["gid"], w, activation=act, **kr)
        s = m["node_score"].detach().numpy().reshape(-1)
        for gid in np.unique(g["gid"]):
            v = np.sort(s[g["gid"] == gid])
            if v.size > 1:
                worst = min(worst, float(np.diff(v).min()))
    return worst


def run_reference():
    tfg, tf, tfs, backend = load_reference()
    R = types.SimpleNamespace(tfg=tfg, tf=tf, tfs=tfs)
    blob = {"__backend__": np.array(backend)}
    for case in ac.CASES:
        g = case.inputs()
        if case.name == "asap":
            gap = min_score_gap(g)
            if not gap >= ac.MIN_SCORE_GAP:
                raise SystemExit("node scores {:.3e} apart inside a graph (< {}): change asap_cases.WEIGHT_SEED or BATCH_SEED".format(
                    gap, ac.MIN_SCORE_GAP))
        for k, v in case.ref(R, g).items():
            blob["{}::{}".format(case.name, k)] = np.asarray(v)
        blob["{}::__inputs_sha256__".format(case.name)] = np.array(inputs_digest(g))
    return blob


if __name__ == "__main__":
    blob = run_reference()
    np.savez_compressed(OUT, **blob)
    print("wrote {} ({} arrays, {} bytes)".format(OUT, len(blob), os.path.getsize(OUT)))
