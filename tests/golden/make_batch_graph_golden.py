# coding=utf-8
"""Writes tests/golden/batch_graph_cases.npz: what the reference's OWN Graph casts and BatchGraph.from_graphs make of the
constructor arguments of tests/batch_graph_cases.py (numpy graphs), run unmodified through oracle/ref_harness (on the numpy
stand-ins for TensorFlow / tf_sparse where those are not installed; the backend is recorded as ``__backend__``).  A digest of
every case's inputs is stored next to the outputs (``<case>::__inputs_sha256__``).  Data only goes into the file.

    python tests/golden/make_batch_graph_golden.py          # regenerate (needs the reference checkout)
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.ref_harness import load_reference   # noqa: E402
import batch_graph_cases as bc                   # noqa: E402

OUT = os.path.join(HERE, "batch_graph_cases.npz")


def inputs_digest(graphs):
    h = hashlib.sha256()
    for i, g in enumerate(graphs):
        for k in sorted(g):
            v = np.asarray(g[k])
            h.update("{}::{}::{}::{}::{}".format(i, k, type(g[k]).__name__, v.dtype, v.shape).encode())
            h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def run_reference(name):
    tfg, _, _, _ = load_reference()
    return bc.run(tfg.Graph, tfg.BatchGraph, bc.CASES[name]())


if __name__ == "__main__":
    blob = {"__backend__": np.array(load_reference()[3])}
    for name in bc.CASES:
        for k, v in run_reference(name).items():
            blob["{}::{}".format(name, k)] = v
        blob["{}::__inputs_sha256__".format(name)] = np.array(inputs_digest(bc.CASES[name]()))
    np.savez_compressed(OUT, **blob)
    print("wrote {} ({} arrays, {} bytes)".format(OUT, len(blob), os.path.getsize(OUT)))
