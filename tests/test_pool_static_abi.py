# coding=utf-8
"""include/tfgx_pool_static.h (one fixed-shape SAGPool level) without a GPU: its names and macros, every argument refusal and
every zero-size success of its entry points; the numpy mirror (tests/sagpool_static_mirror.py) held to the reference's own
recorded sag_pool outputs (tests/golden/pool_cases.npz) and shown to assemble plans that ARE the stable sorts of its emitted
lists, over two levels; the capacity bound of StaticBatchGraph.pooled_capacities brute-forced against the float32 rule.
(The header / table / version / struct checks are tests/test_abi_registry.py's.)"""
import ctypes
import fractions
import os

import numpy as np
import pytest

from abi_header import declarations, macro, refused
from conftest import ROOT
from sagpool_static_mirror import (CLAMPED, MAX_GRAPH_NODES, TOO_LONG, descending_bits, mirror_pooled_capacities,
                                   mirror_sag_pool_static, mirror_topk_static, node_k)
from test_collate_abi import random_dataset
from test_collate_static_abi import mirror_collate_static
from test_drop_edge_abi import mirror_plan

HEADER = "tfgx_pool_static.h"
RATIOS = (0.0, 0.1, 0.25, 0.3, 0.5, 0.7, 1.0, 1.5)


# ---- names and constants ----------------------------------------------------------------------------------------------------
def test_pool_static_names_and_constants():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.STATIC_POOL_SIGNATURES) == [
        "tfgx_static_pool_edges", "tfgx_static_pool_edges_workspace_bytes", "tfgx_static_pool_gather_scale_rows_f32",
        "tfgx_static_pool_select", "tfgx_static_pool_table", "tfgx_static_pool_version"]
    for abi in L.ABIS:
        assert abi.signatures is L.STATIC_POOL_SIGNATURES or not any("static_pool" in n for n in abi.signatures), abi.header
    assert macro(HEADER, "TFGX_STATIC_POOL_MAX_GRAPH_NODES") == L.STATIC_POOL_MAX_GRAPH_NODES == MAX_GRAPH_NODES == 4096
    assert macro(HEADER, "TFGX_STATIC_POOL_CLAMPED") == L.STATIC_POOL_CLAMPED == CLAMPED
    assert macro(HEADER, "TFGX_STATIC_POOL_TOO_LONG") == L.STATIC_POOL_TOO_LONG == TOO_LONG
    assert macro(HEADER, "TFGX_STATIC_POOL_MAX_SLOTS") == L.STATIC_POOL_MAX_SLOTS == L.COLLATE_STATIC_MAX_SLOTS
    # the new flags are not the parent's
    assert not {CLAMPED, TOO_LONG} & {L.COLLATE_STATIC_BAD_ID, L.COLLATE_STATIC_OVERFLOW}
    assert macro("tfgx.h", "TFGX_ABI_VERSION") == L.ABI_VERSION == 114


# ---- refusals and zero-size calls ---------------------------------------------------------------------------------------------
TABLE_OK = dict(graph_row_ptr=1 << 30, parent_counts=2 << 30, B=8, k=-1, ratio=0.5, m_max=60, n_cap_out=64, pooled_row_ptr=3 << 30,
                counts=4 << 30, stream=None)
SELECT_OK = dict(score=1 << 30, graph_row_ptr=2 << 30, pooled_row_ptr=3 << 30, B=8, n_cap=104, sinks=4, n_cap_out=64,
                 node_index=4 << 30, node_graph_index=5 << 30, node_map=6 << 30, stream=None)
GATHER_OK = dict(x=1 << 30, ldx=8, n=104, idx=2 << 30, s=3 << 30, M=64, F=8, out=4 << 30, ldo=8, stream=None)
FAKE = dict(row=1 << 30, col=2 << 30, w=3 << 30, edge_graph_index=4 << 30, n_cap=104, e_cap=120, B=8, sinks=4, sink_degree=32,
            node_map=5 << 30, node_index=6 << 30, pooled_row_ptr=7 << 30, n_cap_out=64, out_row=8 << 30, out_col=9 << 30,
            out_edge_id=10 << 30, out_edge_graph_index=11 << 30, out_w=12 << 30, counts=13 << 30, workspace=14 << 30,
            workspace_bytes=1 << 24)
FAKE_PLAN = dict(ds_row_ptr=15 << 30, ds_col=16 << 30, ds_perm=17 << 30, out_row_ptr=18 << 30, out_col=19 << 30, out_perm=20 << 30)


def _edges(lib, plan=FAKE_PLAN, plan_t=FAKE_PLAN, **kw):
    from tf_geometric_amd import _lib as L
    a = L.StaticPoolArgs(**dict(FAKE, **kw))
    keep = []
    for name, p in (("plan", plan), ("plan_t", plan_t)):
        if p is not None:
            keep.append(L.CollatePlan(**p))
            setattr(a, name, ctypes.pointer(keep[-1]))
    return lib.tfgx_static_pool_edges(ctypes.byref(a), None)


def test_pool_static_argument_validation_without_gpu():
    """Every refusal returns TFGX_ERR_INVALID_ARG (1) on the host, before any device work (the pointers are not memory), with
    the entry point and the argument named."""
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    T = "tfgx_static_pool_table"
    for name in ("B", "m_max", "n_cap_out"):
        refused(T, TABLE_OK, {name: -1}, "negative size (" + name)
        refused(T, TABLE_OK, {name: 1 << 31}, name + " = 2147483648 does not fit int32")
    refused(T, TABLE_OK, dict(B=L.STATIC_POOL_MAX_SLOTS + 1), "B = 1048577 is more than the 1048576 slots")
    refused(T, TABLE_OK, dict(n_cap_out=59), "n_cap_out = 59 is smaller than m_max = 60")
    refused(T, TABLE_OK, dict(ratio=-0.5), "ratio = -0.5 must be at least 0")
    refused(T, TABLE_OK, dict(ratio=float("nan")), "must be at least 0")
    for name in ("graph_row_ptr", "parent_counts", "pooled_row_ptr", "counts"):
        refused(T, TABLE_OK, {name: None}, name + " is null")
    refused(T, TABLE_OK, dict(B=0, counts=None), "counts is null")
    S = "tfgx_static_pool_select"
    for name in ("B", "n_cap", "sinks", "n_cap_out"):
        refused(S, SELECT_OK, {name: -1}, "negative size (" + name)
        refused(S, SELECT_OK, {name: 1 << 31}, name + " = 2147483648 does not fit int32")
    refused(S, SELECT_OK, dict(B=L.STATIC_POOL_MAX_SLOTS + 1), "B = 1048577 is more than the 1048576 slots")
    refused(S, SELECT_OK, dict(sinks=105), "sinks = 105 is more than n_cap = 104")
    for name in ("score", "graph_row_ptr", "pooled_row_ptr", "node_index", "node_graph_index", "node_map"):
        refused(S, SELECT_OK, {name: None}, name + " is null")
    Gt = "tfgx_static_pool_gather_scale_rows_f32"
    for name in ("n", "M", "F"):
        refused(Gt, GATHER_OK, {name: -1}, "negative size (" + name)
    refused(Gt, GATHER_OK, dict(ldx=7), "ldx is smaller than F")
    refused(Gt, GATHER_OK, dict(ldo=7), "ldo is smaller than F")
    refused(Gt, GATHER_OK, dict(n=0), "n must be at least 1")
    for name in ("x", "idx", "out"):
        refused(Gt, GATHER_OK, {name: None}, name + " is null")

    def edges_refused(rc, word, code=1):
        assert rc == code, rc
        msg = lib.tfgx_last_error()
        assert word in msg and b"tfgx_static_pool_edges:" in msg, (word, msg)

    edges_refused(lib.tfgx_static_pool_edges(None, None), b"args is null")
    for member in ("n_cap", "e_cap", "B", "sinks", "sink_degree", "n_cap_out"):
        edges_refused(_edges(lib, **{member: -1}), b"negative size (" + member.encode())
        edges_refused(_edges(lib, **{member: 1 << 31}), member.encode() + b" = 2147483648 does not fit int32")
    edges_refused(_edges(lib, sink_degree=0), b"sink_degree = 0 must be at least 1")
    edges_refused(_edges(lib, sinks=65), b"sinks = 65 is more than n_cap_out = 64")
    edges_refused(_edges(lib, sinks=20, n_cap=10), b"sinks = 20 is more than n_cap = 10")
    edges_refused(_edges(lib, sinks=3), b"sinks = 3 of sink_degree = 32 cannot hold a tail of e_cap = 120")
    for member in ("counts", "pooled_row_ptr", "workspace", "node_map", "node_index", "row", "col", "edge_graph_index", "out_row",
                   "out_col", "out_edge_id", "out_edge_graph_index"):
        edges_refused(_edges(lib, **{member: None}), member.encode() + b" is null")
    edges_refused(_edges(lib, plan=None), b"plan is null")
    edges_refused(_edges(lib, plan_t=None), b"plan_t is null")
    for member in FAKE_PLAN:
        p = dict(FAKE_PLAN, **{member: None})
        edges_refused(_edges(lib, plan=p), b"plan->" + member.encode() + b" is null")
        edges_refused(_edges(lib, plan_t=p), b"plan_t->" + member.encode() + b" is null")
    need = lib.tfgx_static_pool_edges_workspace_bytes(64, 120)
    assert need > 0 and lib.tfgx_static_pool_edges_workspace_bytes(-1, 5) == 0
    edges_refused(_edges(lib, workspace_bytes=need - 1), b"workspace_bytes", code=3)      # TFGX_ERR_WORKSPACE


def test_pool_static_zero_size_calls_succeed_without_gpu():
    """Where nothing exists to be written nothing is launched."""
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    ok = lambda rc: rc == 0 or pytest.fail(lib.tfgx_last_error().decode())      # noqa: E731
    ok(lib.tfgx_static_pool_table(*dict(TABLE_OK, B=0, graph_row_ptr=None, parent_counts=None, pooled_row_ptr=None,
                                        counts=None).values()))
    ok(lib.tfgx_static_pool_select(*dict(SELECT_OK, n_cap=0, sinks=0, n_cap_out=0, score=None, graph_row_ptr=None,
                                         pooled_row_ptr=None, node_index=None, node_graph_index=None, node_map=None).values()))
    for change in (dict(M=0), dict(F=0, ldx=0, ldo=0)):
        ok(lib.tfgx_static_pool_gather_scale_rows_f32(*dict(GATHER_OK, x=None, idx=None, s=None, out=None, **change).values()))
    nothing = {k: None for k, v in FAKE.items() if v >= 1 << 30}
    ok(_edges(lib, plan=None, plan_t=None, **dict(nothing, n_cap=0, e_cap=0, sinks=0, n_cap_out=0, workspace_bytes=0)))


# ---- the mirror is the reference's sag_pool ---------------------------------------------------------------------------------------
def _golden_parent(g, sink_degree=32):
    """The batch of tests/pool_cases.py as a static parent: nodes stably sorted by graph id (ties keep their input order, so the
    selection is the reference's), the gaps as empty slots, the padding of collate_static around it."""
    gid = g["gid"].astype(np.int64)
    order = np.argsort(gid, kind="stable")
    new_of = np.empty_like(order)
    new_of[order] = np.arange(order.size)
    B, n, e = int(gid.max()) + 1, int(g["n"]), int(g["ei"].shape[1])
    P = max(1, -(-e // sink_degree))
    n_cap = n + P
    ei = new_of[g["ei"].astype(np.int64)].astype(np.int32)
    grp = np.concatenate([[0], np.cumsum(np.bincount(gid, minlength=B)), [n_cap]]).astype(np.int32)
    pad = lambda a, fill: np.concatenate([a, np.full((n_cap - n,) + a.shape[1:], fill, a.dtype)])      # noqa: E731
    nodes = np.arange(n_cap, dtype=np.int32)
    # no padded edge: e_cap = e; dead rows (the sinks) own none, so the plans are those of the live list over n_cap rows
    return {"x": pad(g["x"][order], 0), "score": pad(g["score"].reshape(-1)[order], 0), "edge_index": ei, "edge_weight": g["w"],
            "edge_graph_index": gid[g["ei"][0]].astype(np.int32), "graph_mask": np.ones(B, bool),
            "counts": np.asarray([B, n, e, 0], np.int32), "sinks": P, "n_cap": n_cap, "e_cap": e,
            "plan": mirror_plan(ei, n_cap), "plan_t": mirror_plan(ei[[1, 0]], n_cap), "graph_plan": (grp, nodes, nodes)}, B


@pytest.mark.parametrize("name, kr, act, weighted", [("fixed-k3-tanh-w", dict(k=3), "tanh", True),
                                                      ("fixed-ratio-none-w", dict(ratio=0.5), None, True),
                                                      ("fixed-k3-none-now", dict(k=3), None, False)])
def test_mirror_live_part_is_the_recorded_sag_pool(name, kr, act, weighted):
    from pool_cases import batch
    golden = dict(np.load(os.path.join(ROOT, "tests", "golden", "pool_cases.npz")))
    g = batch()
    parent, B = _golden_parent(g)
    if not weighted:
        parent["edge_weight"] = np.ones_like(parent["edge_weight"])
    score = parent["score"]
    scale = np.tanh(score) if act == "tanh" else score
    m = mirror_sag_pool_static(parent, B, 32, score, x=parent["x"], scale=scale, **kr)
    ref = {k.split("/")[1]: v for k, v in golden.items() if k.startswith("sag_pool::" + name + "/")}
    m_live, e_kept = m["n_live"], m["e_live"]
    assert (m_live, e_kept) == (ref["x"].shape[0], ref["edge_index"].shape[1]) and m["counts"].tolist() == [B, m_live, e_kept, 0]
    assert np.array_equal(m["edge_index"][:, :e_kept], ref["edge_index"])
    assert np.array_equal(m["node_graph_index"][:m_live], ref["node_graph_index"])
    assert np.array_equal(m["edge_weight"][:e_kept], ref["edge_weight"])
    if act is None:
        assert np.array_equal(m["x"][:m_live], ref["x"])
    else:
        assert np.abs(m["x"][:m_live] - ref["x"]).max() <= 1e-5          # tanh: libm ulps (tests/pool_cases.py)
    assert not m["x"][m_live:].any() and (m["node_index"][m_live:] == -1).all() and (m["edge_id"][e_kept:] == -1).all()


# ---- the mirror's plans are the stable sorts of its lists, over two levels ------------------------------------------------------
SIZES = [(3, 4), (0, 0), (5, 0), (2, 6), (1, 1), (0, 0), (7, 20), (40, 100), (33, 70), (65, 150)]
BATCHES = {"all live": list(range(len(SIZES))), "dead first": [-1, 3, 6], "dead in the middle": [7, -1, -1, 9], "dead last": [8, 3, -1],
           "only dead": [-1, -1, -1], "a graph three times": [6, 6, 6], "empty graphs": [1, 5, 1], "no slot": [], "one": [9]}
SELECTIONS = (dict(k=1), dict(k=3), dict(k=1000), dict(ratio=0.0), dict(ratio=0.3), dict(ratio=0.5), dict(ratio=1.0), dict(ratio=1.5))


@pytest.mark.parametrize("sink_degree", [1, 32])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_mirror_plans_are_the_stable_sorts_of_its_lists_over_two_levels(name, sink_degree):
    rng = np.random.Generator(np.random.PCG64(5))
    d = random_dataset(rng, SIZES, 5)
    ids = BATCHES[name]
    B = len(ids)
    parent0 = mirror_collate_static(d["x"], d["edge_index"], d["edge_weight"], d["node_ptr"], d["edge_ptr"], ids, sink_degree=sink_degree)
    for kr in SELECTIONS:
        parent = parent0
        for level in range(2):
            n_cap, e_cap, P = parent["n_cap"], parent["e_cap"], parent["sinks"]
            score = (np.round(rng.standard_normal(n_cap) * 2.0) / 2.0).astype(np.float32)      # halves: many ties
            x = rng.standard_normal((n_cap, 3)).astype(np.float32)
            m = mirror_sag_pool_static(parent, B, sink_degree, score, x=x, **kr)
            what = (name, sink_degree, kr, level)
            n_out, m_live, e_kept = m["n_cap"], m["n_live"], m["e_live"]
            assert m["e_cap"] == e_cap and m["sinks"] == P and n_out == mirror_pooled_capacities(n_cap - P, B, **kr) + P
            assert not m["counts"][3] & (CLAMPED | TOO_LONG)
            for key, ei in (("plan", m["edge_index"]), ("plan_t", m["edge_index"][[1, 0]])):
                for got, ref, part in zip(m[key], mirror_plan(ei, n_out), ("row_ptr", "col", "perm")):
                    assert np.array_equal(got, ref) and got.dtype == ref.dtype, what + (key, part)
            ref = mirror_plan(np.stack([m["node_graph_index"], np.arange(n_out, dtype=np.int32)]), B + 1)
            for got, r, part in zip(m["graph_plan"], ref, ("row_ptr", "col", "perm")):
                assert np.array_equal(got, r), what + ("graph_plan", part)
            # the padding is inert, as the parent's
            assert not m["x"][m_live:].any() and (m["node_graph_index"][m_live:] == B).all() and m_live <= n_out - P
            assert (m["edge_index"][:, :e_kept] < m_live).all() and (m["edge_index"][:, e_kept:] >= n_out - P).all()
            assert (m["edge_weight"][e_kept:] == 1.0).all()
            assert np.bincount(m["edge_index"][0, e_kept:], minlength=n_out).max(initial=0) <= sink_degree
            # the selection: per slot the first node_k of a stable descending sort; node_map inverts node_index
            grp = parent["graph_plan"][0]
            for g in range(B):
                rows = np.arange(grp[g], grp[g + 1])
                want = rows[np.argsort(-np.where(score[rows] == 0, 0.0, score[rows]), kind="stable")][:node_k(rows.size, **kr)]
                assert np.array_equal(m["node_index"][m["pooled_row_ptr"][g]:m["pooled_row_ptr"][g + 1]], want), what
            assert np.array_equal(m["node_map"][m["node_index"][:m_live]], np.arange(m_live))
            assert (m["node_map"] >= 0).sum() == m_live
            parent = m


def test_descending_bits_orders_like_a_descending_stable_sort():
    s = np.asarray([0.5, -0.0, 0.0, -1.5, np.inf, -np.inf, 0.5, 3.0, -0.0, 1e-40, -1e-40], np.float32)
    order = np.argsort(descending_bits(s), kind="stable")
    assert order.tolist() == [4, 7, 0, 6, 9, 1, 2, 8, 10, 3, 5]
    # a NaN with the sign bit clear sorts before +inf, as in the radix key of tfgx_segment_topk
    assert np.argsort(descending_bits(np.asarray([1.0, np.float32("nan"), np.inf], np.float32)), kind="stable").tolist()[-2:] == [2, 0]


# ---- the capacity bound -------------------------------------------------------------------------------------------------------
def test_per_graph_inequality_of_the_float32_rule():
    """k_g <= n_g, and k_g < float32(ratio) * n_g * (1 + 2^-22) + 1 in exact arithmetic: what the proof of the bound uses."""
    slack = 1 + fractions.Fraction(1, 1 << 22)
    for ratio in RATIOS:
        r = fractions.Fraction(float(np.float32(ratio)))
        for n in range(0, 4101):
            kg = node_k(n, ratio=ratio)
            assert 0 <= kg <= n and kg < r * n * slack + 1, (ratio, n, kg)
    for k in (0, 1, 3, 1000):
        assert all(node_k(n, k=k) == min(k, n) for n in range(0, 4101))


def _static_batch(B, max_nodes, max_edges=64, sink_degree=32):
    """A StaticBatchGraph that holds capacities only (pooled_capacities is host arithmetic on them)."""
    import torch
    import tf_geometric_amd as tfg
    P = max(1, -(-max_edges // sink_degree))
    cap = tfg.data.StaticBatchCapacities(B, max_nodes, max_edges, sink_degree, P, max_nodes + P, max_edges)
    z = torch.zeros(0, dtype=torch.int32)
    return tfg.data.StaticBatchGraph(torch.zeros((0, 1)), torch.zeros((2, 0), dtype=torch.int32), z, z, None, None, z,
                                     torch.zeros(B, dtype=torch.bool), torch.zeros(4, dtype=torch.int32), cap, 0)


def test_sum_of_kept_nodes_is_within_m_max_for_random_multisets():
    rng = np.random.Generator(np.random.PCG64(11))
    tight = 0
    for trial in range(3000):
        B = int(rng.integers(1, 40))
        hi = int(rng.choice([4, 60, 300, 4100]))
        sizes = rng.integers(0, hi + 1, int(rng.integers(0, B + 1)))          # the live graphs: at most B
        max_nodes = int(sizes.sum()) + int(rng.integers(0, 50)) * int(rng.integers(0, 2))
        for ratio in RATIOS:
            m_max = mirror_pooled_capacities(max_nodes, B, ratio=ratio)
            total = sum(node_k(int(n), ratio=ratio) for n in sizes)
            assert total <= m_max <= max_nodes, (trial, ratio, total, m_max)
            tight += total == m_max
        for k in (0, 1, 3, 1000):
            assert sum(node_k(int(n), k=k) for n in sizes) <= mirror_pooled_capacities(max_nodes, B, k=k) <= max_nodes
        if trial % 100 == 0:                                                  # the package computes the mirror's number
            batch = _static_batch(B, max_nodes)
            for ratio in RATIOS:
                cap = batch.pooled_capacities(ratio=ratio)
                assert cap.max_nodes == mirror_pooled_capacities(max_nodes, B, ratio=ratio)
                assert (cap.batch_size, cap.max_edges, cap.sink_degree, cap.sinks, cap.e_cap) == (B, 64, 32, 2, 64)
                assert cap.n_cap == cap.max_nodes + cap.sinks
            for k in (0, 1, 3, 1000):
                assert batch.pooled_capacities(k=k).max_nodes == min(max_nodes, B * k)
    assert tight > 0, "the bound is reached by some multiset (ratio 1.0 keeps every node)"


def test_pooled_capacities_refusals():
    batch = _static_batch(4, 100)
    for kw, word in ((dict(), "got neither"), (dict(k=2, ratio=0.5), "not both"), (dict(k=-1), "k must be an integer"),
                     (dict(k=1.5), "k must be an integer"), (dict(k=True), "k must be an integer"), (dict(k=1 << 31), "does not fit int32"),
                     (dict(ratio=-0.1), "at least 0"), (dict(ratio=float("nan")), "at least 0"), (dict(ratio=float("inf")), "finite"),
                     (dict(ratio="half"), "ratio must be a number")):
        with pytest.raises(ValueError, match="pooled_capacities: .*" + word):
            batch.pooled_capacities(**kw)
    big = _static_batch(4, (1 << 31) - 3, max_edges=64)
    with pytest.raises(ValueError, match="do not fit int32"):
        big.pooled_capacities(ratio=1.0)


def test_static_pooling_needs_a_gpu_and_refuses_on_the_host_first():
    import torch
    import tf_geometric_amd as tfg
    with pytest.raises(ValueError, match="batch must be a StaticBatchGraph"):
        tfg.nn.sag_pool_static(torch.zeros((3, 2)), object(), lambda *a, **k: None, ratio=0.5)
    with pytest.raises(ValueError, match="does not come from GraphStore.collate_static"):
        tfg.nn.topk_pool_static(_static_batch(2, 10), torch.zeros(11), k=1)
