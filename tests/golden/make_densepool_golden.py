# coding=utf-8
"""Writes tests/golden/densepool_cases.npz: the outputs of the reference's OWN diff_pool, diff_pool_coarsen,
min_cut_pool(return_losses=True), min_cut_pool_coarsen and min_cut_pool_compute_losses on the inputs of
tests/densepool_cases.py, run unmodified through oracle/ref_harness (on the numpy stand-ins for TensorFlow / tf_sparse where
those are not installed; the backend is recorded as ``__backend__``).  On the stand-ins the loss runs with the three adapters
of densepool_cases.install_adapters.  A digest of the inputs is stored next to the outputs.

The generator refuses inputs on which the set of non-zero pooled entries could be a float32 accident: every assign logit
(from the float64 mirror, tests/densepool_mirror.py) must stay within densepool_cases.MAX_LOGIT and every in-block pooled
entry of a graph that has an edge must be at least densepool_cases.MIN_ENTRY; change the seed of densepool_cases.batch when
it fails.

    python tests/golden/make_densepool_golden.py          # regenerate (needs the reference checkout)
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
import densepool_cases as dc                     # noqa: E402
from make_pool_golden import inputs_digest       # noqa: E402

OUT = os.path.join(HERE, "densepool_cases.npz")


def reference():
    tfg, tf, tfs, backend = load_reference()
    return types.SimpleNamespace(tfg=tfg, tf=tf, tfs=tfs, backend=backend)


def run_reference():
    R = reference()
    blob = {"__backend__": np.array(R.backend)}
    for case in dc.CASES:
        g = case.inputs()
        big, small = dc.checks(g)
        if not (big <= dc.MAX_LOGIT and small >= dc.MIN_ENTRY):
            raise SystemExit("largest |logit| {:.3f} (limit {}), smallest in-block entry {:.3e} (limit {}): change the seed of "
                             "densepool_cases.batch".format(big, dc.MAX_LOGIT, small, dc.MIN_ENTRY))
        for k, v in case.ref(R, g).items():
            blob["{}::{}".format(case.name, k)] = np.asarray(v)
        blob["{}::__inputs_sha256__".format(case.name)] = np.array(inputs_digest(g))
    return blob


if __name__ == "__main__":
    blob = run_reference()
    np.savez_compressed(OUT, **blob)
    print("wrote {} ({} arrays, {} bytes)".format(OUT, len(blob), os.path.getsize(OUT)))
