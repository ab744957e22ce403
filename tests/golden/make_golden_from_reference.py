# coding=utf-8
"""Writes tests/golden/reference_cases.npz: the outputs of the reference's OWN Python on the inputs of
tests/reference_cases.py.

The reference (``/root/reference/tf_geometric``, v0.1.7) is imported UNMODIFIED by oracle/ref_harness.  With real
``tensorflow`` + ``tf_sparse`` installed they are used; in this image they are not installable, so the reference
runs on the numpy stand-ins of oracle/ref_harness/stubs (restated TF / tf_sparse primitives; the composition logic —
every line of tf_geometric — is the reference's).  The backend used is recorded in the file (``__backend__``).

    python tests/golden/make_golden_from_reference.py          # regenerate (needs /root/reference)

It also writes tests/golden/reference_checks.npz (``checks`` alone: ``python tests/golden/make_golden_from_reference.py
checks``): what tests/test_oracle_vs_reference.py reads where the reference checkout is absent — the hashes of the
reference files the harness loads, a digest of every case's inputs, the reference's outputs on the fuzz seeds and its
split-size table.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.ref_harness import load_reference   # noqa: E402
import reference_cases as rc                     # noqa: E402

OUT = os.path.join(HERE, "reference_cases.npz")
OUT_CHECKS = os.path.join(HERE, "reference_checks.npz")


def run_reference():
    tfg, tf, tfs, backend = load_reference()
    R = types.SimpleNamespace(tfg=tfg, tf=tf, tfs=tfs)
    blob = {"__backend__": np.array(backend), "__reference_version__": np.array("tf_geometric 0.1.7")}
    for case in rc.CASES:
        outs = case.ref(R, case.inputs())
        for k, v in outs.items():
            blob["{}::{}".format(case.name, k)] = np.asarray(v)
        print("{:<28s} {:3d} outputs".format(case.name, len(outs)))
    return blob


def run_checks():
    import hashlib
    import json
    from oracle.ref_harness.load_reference import REFERENCE_ROOT
    tfg, tf, tfs, backend = load_reference()
    R = types.SimpleNamespace(tfg=tfg, tf=tf, tfs=tfs)
    blob = {"__backend__": np.array(backend)}
    for rel in rc.REFERENCE_FILES:
        with open(os.path.join(REFERENCE_ROOT, "tf_geometric", rel), "rb") as fh:
            blob["sha1::" + rel] = np.array(hashlib.sha1(fh.read()).hexdigest())
    for case in rc.CASES:
        blob["inputs_sha256::" + case.name] = np.array(rc.inputs_digest(case.inputs()))
    for seed in rc.FUZZ_SEEDS:
        for k, v in rc.fuzz_check_ref(R, rc.fuzz_check_inputs(seed)).items():
            blob["fuzz{}::{}".format(seed, k)] = np.asarray(v)
    blob["num_splits"] = np.array(json.dumps(rc.num_splits_table(tfg.utils.tf_sparse_utils.compute_num_or_size_splits)))
    return blob


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    for name, out, run in (("cases", OUT, run_reference), ("checks", OUT_CHECKS, run_checks)):
        if what not in ("all", name):
            continue
        blob = run()
        np.savez_compressed(out, **blob)
        print("wrote {} ({} arrays, {:.0f} KB, backend = {})".format(out, len(blob), os.path.getsize(out) / 1024.0,
                                                                      blob["__backend__"]))
