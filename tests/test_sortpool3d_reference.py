# coding=utf-8
"""tests/golden/sortpool3d_cases.npz is what the reference's own convert_x_to_3d and sort_pool -> convert_x_to_3d produce on the
inputs of tests/sortpool3d_cases.py, and the numpy mirror (tests/sortpool3d_mirror.py) — the statement the GPU tests hold the
kernel to — reproduces it exactly (no GPU needed).  The live comparison runs where the reference checkout exists."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import sortpool3d_cases as sc
from sortpool3d_mirror import (graph_plan, mirror_backward, mirror_convert_x_to_3d, mirror_rows_3d, mirror_sort_pool_3d)
from sagpool_static_mirror import TOO_LONG

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_sortpool3d_golden as mk     # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "sortpool3d_cases.npz")
CASES = pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_golden_file_is_small():
    assert os.path.getsize(GOLDEN) < 1 << 20


@CASES
def test_golden_inputs_are_the_case_table(case, golden):
    """The committed outputs were produced from exactly the inputs the case table builds today."""
    assert str(golden["{}::__inputs_sha256__".format(case.name)]) == mk.inputs_digest(case.inputs())
    assert any(k.startswith(case.name + "::") and not k.endswith("__") for k in golden)


@CASES
def test_sort_columns_are_distinct_within_every_graph(case):
    g = case.inputs()
    for gid in np.unique(g["gid"]):
        rows = g["x"][g["gid"] == gid]
        assert all(np.unique(rows[:, c]).size == rows.shape[0] for c in range(rows.shape[1]))


@CASES
def test_mirror_equals_the_reference(case, golden):
    g = case.inputs()
    n_ref = int(g["gid"].max()) + 1
    for name, k, pad, si in case.configs:
        for num in sc.NUM_SOURCES[case.name]:
            ref = golden["{}::{}/convert".format(case.name, name)]
            got, slot_node, node_slot = mirror_convert_x_to_3d(g["x"], g["gid"], k=k, pad=pad, num_sources=num, with_index=True)
            assert got.dtype == ref.dtype == np.float32 and got.shape == ((num or n_ref),) + ref.shape[1:], name
            assert np.array_equal(got[:n_ref], ref) and not got[n_ref:].any(), name
            _check_index(g["x"], got, slot_node, node_slot)
            if k is not None and pad:
                ref = golden["{}::{}/sort".format(case.name, name)]
                got, slot_node, node_slot, flags = mirror_sort_pool_3d(g["x"], g["gid"], k, sort_index=si, num_graphs=num,
                                                                       with_index=True)
                assert got.shape == ((num or n_ref),) + ref.shape[1:] and flags == 0, name
                assert np.array_equal(got[:n_ref], ref) and not got[n_ref:].any(), name
                _check_index(g["x"], got, slot_node, node_slot)


def _check_index(x, out, slot_node, node_slot):
    """slot_node and node_slot are each other's inverse, and out is x through slot_node."""
    rows = out.reshape(-1, out.shape[-1])
    live = slot_node >= 0
    assert np.array_equal(rows[live], x[slot_node[live]]) and not rows[~live].any()
    assert np.array_equal(node_slot[slot_node[live]], np.flatnonzero(live))
    assert (node_slot >= 0).sum() == live.sum()
    d = np.arange(rows.size, dtype=np.float32).reshape(rows.shape) + 1.0
    dx = mirror_backward(d, node_slot)
    assert np.array_equal(dx[slot_node[live]], d[live]) and not dx[node_slot < 0].any()


def test_mirror_flags_a_graph_above_the_cap_and_keeps_none_of_it():
    x = np.arange(12, dtype=np.float32).reshape(6, 2)
    seg_ptr, seg_node = graph_plan([0, 1, 1, 1, 1, 0], 2)
    out, slot_node, node_slot, flags = mirror_rows_3d(x, seg_ptr, seg_node, 2, 3, sort_col=1, cap=3)
    assert flags == TOO_LONG and not out[3:].any() and (slot_node[3:] == -1).all()
    assert node_slot.tolist() == [1, -1, -1, -1, -1, 0] and slot_node[:3].tolist() == [5, 0, -1]
    # the plain mode has no cap
    assert mirror_rows_3d(x, seg_ptr, seg_node, 2, 3, cap=3)[3] == 0


def test_mirror_ties_nan_and_zero_follow_the_topk_key():
    """Equal keys keep plan order, -0.0 equals +0.0, a NaN of either sign sorts by its bits (positive first, negative last)."""
    key = np.array([1.0, -0.0, 0.0, 1.0, np.nan, -np.inf, np.inf, -np.nan], dtype=np.float32)
    x = np.stack([np.arange(8, dtype=np.float32), key], axis=1)
    _, slot_node, _, _ = mirror_sort_pool_3d(x, np.zeros(8, dtype=np.int32), 8, sort_index=1, with_index=True)
    pos_nan, neg_nan = (4, 7) if not np.signbit(key[4]) else (7, 4)
    assert slot_node.tolist() == [pos_nan, 6, 0, 3, 1, 2, 5, neg_nan]


@CASES
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
