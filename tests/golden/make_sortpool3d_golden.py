# coding=utf-8
"""Writes tests/golden/sortpool3d_cases.npz: the outputs of the reference's OWN convert_x_to_3d and sort_pool ->
convert_x_to_3d on the inputs of tests/sortpool3d_cases.py, run unmodified through oracle/ref_harness (on the numpy stand-ins
for TensorFlow / tf_sparse where those are not installed; the backend is recorded as ``__backend__``).  A digest of every case's
inputs is stored next to the outputs (``<case>::__inputs_sha256__``).

    python tests/golden/make_sortpool3d_golden.py          # regenerate (needs the reference checkout)
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
from make_pool_golden import inputs_digest       # noqa: E402
import sortpool3d_cases as sc                    # noqa: E402

OUT = os.path.join(HERE, "sortpool3d_cases.npz")


def run_reference():
    tfg, tf, tfs, backend = load_reference()
    R = types.SimpleNamespace(tfg=tfg, tf=tf, tfs=tfs)
    blob = {"__backend__": np.array(backend)}
    for case in sc.CASES:
        g = case.inputs()
        for k, v in case.ref(R, g).items():
            blob["{}::{}".format(case.name, k)] = np.asarray(v)
        blob["{}::__inputs_sha256__".format(case.name)] = np.array(inputs_digest(g))
    return blob


if __name__ == "__main__":
    blob = run_reference()
    np.savez_compressed(OUT, **blob)
    print("wrote {} ({} arrays, {} bytes)".format(OUT, len(blob), os.path.getsize(OUT)))
