# coding=utf-8
"""tests/golden/pool_cases.npz is what the reference's own sag_pool / sort_pool / sample_new_graph_by_node_index produce on
the inputs of tests/pool_cases.py (no GPU needed).  The live comparison runs where the reference checkout exists."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import pool_cases as pc

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_pool_golden as mk     # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pool_cases.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_golden_file_is_small():
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_golden_inputs_are_the_case_table(case, golden):
    """The committed outputs were produced from exactly the inputs the case table builds today."""
    assert str(golden["{}::__inputs_sha256__".format(case.name)]) == mk.inputs_digest(case.inputs())
    assert any(k.startswith(case.name + "::") and not k.endswith("__") for k in golden)


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_golden_file_is_what_the_reference_produces(case, golden):
    from oracle.ref_harness import reference_available
    if not reference_available():
        pytest.skip("reference checkout not present")
    import types
    from oracle.ref_harness import load_reference
    tfg, tf, tfs, _ = load_reference()
    outs = case.ref(types.SimpleNamespace(tfg=tfg, tf=tf, tfs=tfs), case.inputs())
    keys = [k for k in golden if k.startswith(case.name + "::") and not k.endswith("__")]
    assert sorted(keys) == sorted(case.name + "::" + k for k in outs)
    for k, v in outs.items():
        ref = golden[case.name + "::" + k]
        v = np.asarray(v)
        assert v.dtype == ref.dtype and v.shape == ref.shape, k
        assert np.array_equal(v, ref), "{}: live reference run differs from the committed golden file".format(k)
