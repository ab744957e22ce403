# coding=utf-8
"""include/tfgx_dense_pool_static.h without a GPU: names and macros against _lib, every refusal (on the host, the argument
named), the zero-size call, the numpy mirror of the layout (tests/densepool_static_mirror.py) against the reference's recorded
diff_pool_coarsen / min_cut_pool_coarsen (tests/golden/densepool_cases.npz), the mirror's closed-form plans against a stable
sort, and StaticBatchGraph.dense_pooled_capacities against brute force."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from abi_header import declarations, macro
from conftest import ROOT
from densepool_static_mirror import mirror_dense_capacities, mirror_dense_pool_static, mirror_pooled_weight
from test_drop_edge_abi import mirror_plan
import densepool_cases as dc

HEADER = "tfgx_dense_pool_static.h"
GOLDEN = os.path.join(ROOT, "tests", "golden", "densepool_cases.npz")


def test_dense_pool_static_names_and_constants():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.DENSE_POOL_STATIC_SIGNATURES) == [
        "tfgx_dense_pool_static", "tfgx_dense_pool_static_version", "tfgx_dense_pool_static_workspace_bytes"]
    for abi in L.ABIS:
        assert abi.signatures is L.DENSE_POOL_STATIC_SIGNATURES or not any("dense_pool" in n for n in abi.signatures), abi.header
    assert macro(HEADER, "TFGX_DENSE_POOL_STATIC_ABI_VERSION") == L.DENSE_POOL_STATIC_ABI_VERSION == 1
    assert L.load_library().tfgx_dense_pool_static_version() == 1
    assert macro(HEADER, "TFGX_DENSE_POOL_STATIC_MAX_K") == L.DENSE_POOL_STATIC_MAX_K == L.SEGGRAM_MAX_K == 64
    assert macro("tfgx_seggram.h", "TFGX_SEGGRAM_MAX_K") == L.DENSE_POOL_STATIC_MAX_K
    assert macro(HEADER, "TFGX_DENSE_POOL_STATIC_MAX_SLOTS") == L.DENSE_POOL_STATIC_MAX_SLOTS == L.STATIC_POOL_MAX_SLOTS
    assert macro("tfgx.h", "TFGX_ABI_VERSION") == L.ABI_VERSION == 114


# B = 8 slots of K = 5 clusters: 40 rows + 7 sinks of degree 32 for 200 edges
FAKE = dict(P=1 << 30, ldp=5, graph_mask=2 << 30, parent_counts=3 << 30, B=8, K=5, drop_diagonal=0, n_cap_out=47, e_cap=200, sinks=7,
            sink_degree=32, pooled_row_ptr=4 << 30, node_index=5 << 30, node_graph_index=6 << 30, node_map=7 << 30, out_row=8 << 30,
            out_col=9 << 30, out_edge_src=10 << 30, out_edge_graph_index=11 << 30, counts=12 << 30, workspace=13 << 30,
            workspace_bytes=1 << 20)
FAKE_PLAN = dict(out_row_ptr=14 << 30, out_col=15 << 30, out_perm=16 << 30)


def _call(lib, plan=FAKE_PLAN, plan_t=FAKE_PLAN, **kw):
    from tf_geometric_amd import _lib as L
    a = L.DensePoolStaticArgs(**dict(FAKE, **kw))
    keep = []
    for name, p in (("plan", plan), ("plan_t", plan_t)):
        if p is not None:
            keep.append(L.CollatePlan(**p))
            setattr(a, name, ctypes.pointer(keep[-1]))
    return lib.tfgx_dense_pool_static(ctypes.byref(a), None)


def test_dense_pool_static_argument_validation_without_gpu():
    """Every refusal returns TFGX_ERR_INVALID_ARG (1) on the host, before any device work (the pointers are not memory), with
    the entry point and the argument named."""
    from tf_geometric_amd import _lib as L
    lib = L.load_library()

    def refused(rc, word, code=1):
        assert rc == code, (rc, word)
        msg = lib.tfgx_last_error()
        assert word in msg and b"tfgx_dense_pool_static:" in msg, (word, msg)

    refused(lib.tfgx_dense_pool_static(None, None), b"args is null")
    for member in ("B", "K", "ldp", "n_cap_out", "e_cap", "sinks", "sink_degree"):
        refused(_call(lib, **{member: -1}), b"negative size (" + member.encode())
        refused(_call(lib, **{member: 1 << 31}), member.encode() + b" = 2147483648 does not fit int32")
    refused(_call(lib, B=L.DENSE_POOL_STATIC_MAX_SLOTS + 1), b"B = 1048577 is more than the 1048576 slots")
    refused(_call(lib, K=0), b"K = 0 is outside [1, 64]")
    refused(_call(lib, K=65, ldp=65), b"K = 65 is outside [1, 64]")
    refused(_call(lib, ldp=4), b"ldp is smaller than K")
    refused(_call(lib, sink_degree=0), b"sink_degree = 0 must be at least 1")
    refused(_call(lib, sinks=6), b"sinks = 6 of sink_degree = 32 cannot hold a tail of e_cap = 200")
    refused(_call(lib, n_cap_out=46), b"n_cap_out = 46 is smaller than B * K + sinks = 47")
    refused(_call(lib, B=1 << 20, K=64, ldp=64, n_cap_out=(1 << 26) + 7), b"B * K * K = 4294967296 does not fit int32")
    for member in ("counts", "parent_counts", "pooled_row_ptr", "workspace", "P", "graph_mask", "node_map", "node_index",
                   "node_graph_index", "out_row", "out_col", "out_edge_src", "out_edge_graph_index"):
        refused(_call(lib, **{member: None}), member.encode() + b" is null")
    refused(_call(lib, plan=None), b"plan is null")
    refused(_call(lib, plan_t=None), b"plan_t is null")
    for member in FAKE_PLAN:
        p = dict(FAKE_PLAN, **{member: None})
        refused(_call(lib, plan=p), b"plan->" + member.encode() + b" is null")
        refused(_call(lib, plan_t=p), b"plan_t->" + member.encode() + b" is null")
    need = lib.tfgx_dense_pool_static_workspace_bytes(8)
    assert need > 0 and lib.tfgx_dense_pool_static_workspace_bytes(-1) == 0
    assert lib.tfgx_dense_pool_static_workspace_bytes(L.DENSE_POOL_STATIC_MAX_SLOTS + 1) == 0
    refused(_call(lib, workspace_bytes=need - 1), b"workspace_bytes", code=3)          # TFGX_ERR_WORKSPACE


def test_dense_pool_static_zero_size_call_succeeds_without_gpu():
    """Where nothing exists to be written nothing is launched."""
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    nothing = {k: None for k, v in FAKE.items() if v >= 1 << 30}
    for K, drop in ((1, 0), (5, 1), (64, 0)):
        rc = _call(lib, plan=None, plan_t=None, **dict(nothing, B=0, K=K, ldp=K, drop_diagonal=drop, n_cap_out=0, e_cap=0, sinks=0,
                                                      workspace_bytes=0))
        assert rc == 0, lib.tfgx_last_error().decode()


# ---- the mirror is the reference's coarsening ------------------------------------------------------------------------------------
def _blocks(g, weighted, normed):
    """S_g^T A_g S_g of the case batch in float64 -> float32 [G K, K]; A from the edge list (no duplicates in the case), for
    min_cut_pool_coarsen normalised as D^-1/2 A D^-1/2 with D the row sums."""
    n, K, G = g["n"], dc.K, len(dc.SIZES)
    A = np.zeros((n, n))
    A[g["ei"][0], g["ei"][1]] = g["w"].astype(np.float64) if weighted else 1.0
    if normed:
        deg = A.sum(axis=1)
        with np.errstate(divide="ignore"):
            dis = np.where(deg > 0, deg ** -0.5, 0.0)
        A = dis[:, None] * A * dis[None, :]
    S = g["assign"].astype(np.float64)
    P = np.zeros((G * K, K))
    for q in range(G):
        nodes = np.flatnonzero(g["gid"] == q)
        P[q * K:(q + 1) * K] = S[nodes].T @ A[np.ix_(nodes, nodes)] @ S[nodes]
    return P.astype(np.float32)


@pytest.mark.parametrize("sink_degree", [1, 32])
@pytest.mark.parametrize("fn,normed", [("diff_pool_coarsen", False), ("min_cut_pool_coarsen", True)])
@pytest.mark.parametrize("name,weighted", dc.COARSEN_CONFIGS)
def test_mirror_live_part_is_the_recorded_coarsening(name, weighted, fn, normed, sink_degree):
    golden = np.load(GOLDEN)
    pre = "densepool::{}/{}/".format(fn, name)
    g = dc.batch()
    K, G = dc.K, len(dc.SIZES)
    P = _blocks(g, weighted, normed)
    for slots in (list(range(G)), [0, -1, 1, 2, -1, 3, 4], [0, 1, 2, 3, 4, -1, -1]):
        # slot j holds graph slots[j]; the blocks of dead slots hold what must not matter
        B = len(slots)
        Ps = np.full((B * K, K), 7.0, np.float32)
        mask = np.asarray([s >= 0 for s in slots])
        for j, s in enumerate(slots):
            if s >= 0:
                Ps[j * K:(j + 1) * K] = P[s * K:(s + 1) * K]
        _, _, sinks, n_cap, e_cap = mirror_dense_capacities(B, K, sink_degree, drop_diagonal=normed)
        m = mirror_dense_pool_static(Ps, mask, [G, 0, 0, 2], K, normed, n_cap, e_cap, sinks, sink_degree)
        e, rows = m["e_live"], m["m_live"]
        assert rows == G * K and list(m["counts"]) == [G, G * K, e, 2]
        assert np.array_equal(m["edge_index"][:, :e], golden[pre + "edge_index"])
        live_slots = np.flatnonzero(mask)
        assert np.array_equal(live_slots[golden[pre + "node_graph_index"]], m["node_graph_index"][:rows])
        w = mirror_pooled_weight(Ps, m["edge_src"])
        ref = golden[pre + "edge_weight"]
        assert np.abs(w[:e] - ref).max() <= 1e-6 * (1.0 + np.abs(ref).max())
        assert (w[e:] == 1.0).all() and (m["edge_src"][e:] == -1).all() and (m["edge_graph_index"][e:] == B).all()
        assert (m["edge_index"][:, e:] >= n_cap - sinks).all() and (m["edge_index"][0, e:] == m["edge_index"][1, e:]).all()
        assert np.bincount(m["edge_index"][0, e:], minlength=n_cap).max(initial=0) <= sink_degree


# ---- the mirror's closed-form plans are stable sorts --------------------------------------------------------------------------
def _random_blocks(rng, B, K, density):
    P = rng.integers(1, 4, (B * K, K)).astype(np.float32) * (rng.random((B * K, K)) < density)
    if P.size >= 2:
        P.reshape(-1)[0], P.reshape(-1)[-1] = -0.0, np.nan
    return P


@pytest.mark.parametrize("sink_degree", [1, 32])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("K", [1, 3, 20, 64])
def test_mirror_plans_are_the_stable_sorts_of_its_list_and_of_the_flip(K, drop, sink_degree):
    rng = np.random.Generator(np.random.PCG64(K * 4 + drop * 2 + sink_degree))
    for mask in ([1, 1, 1, 0, 0], [0, 1, 0, 1, 1, 0], [0, 0, 0], [1], []):
        B = len(mask)
        for density in (0.0, 0.4, 1.0):
            P = _random_blocks(rng, B, K, density)
            _, _, sinks, n_cap, e_cap = mirror_dense_capacities(B, K, sink_degree, drop_diagonal=drop)
            m = mirror_dense_pool_static(P, mask, [sum(mask), 0, 0, 0], K, drop, n_cap, e_cap, sinks, sink_degree)
            ei = m["edge_index"]
            for got, ref in ((m["plan"], mirror_plan(ei, n_cap)), (m["plan_t"], mirror_plan(ei[::-1], n_cap))):
                for a, b in zip(got, ref):
                    assert np.array_equal(a, b)
            e = m["e_live"]
            assert (np.diff(ei[0]) >= 0).all()                   # sorted by row: the plan by row is the list
            live = np.flatnonzero(mask)
            flat = P.reshape(-1)
            kept = flat[m["edge_src"][:e]]
            assert ((kept != 0) | np.isnan(kept)).all()
            if P.size >= 2 and B and mask[0] and not (drop and K == 1):
                assert 0 not in m["edge_src"][:e]                # -0.0 is no edge
            if P.size >= 2 and B and mask[-1] and not drop:
                assert B * K * K - 1 in m["edge_src"][:e]        # a NaN is one
            assert np.array_equal(m["edge_graph_index"][:e], m["edge_src"][:e] // (K * K))
            assert np.isin(m["edge_graph_index"][:e], live).all()


# ---- the capacities ---------------------------------------------------------------------------------------------------------
def _static_batch(B, sink_degree):
    import torch
    from tf_geometric_amd.data import graph as G
    from tf_geometric_amd.data.graph_store import StaticBatchCapacities
    cap = StaticBatchCapacities(B, 7 * B, 9 * B, sink_degree, max(1, -(-9 * B // sink_degree)), 7 * B + max(1, -(-9 * B // sink_degree)),
                                9 * B)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)      # noqa: E731
    return G.StaticBatchGraph(torch.zeros((cap.n_cap, 1)), torch.zeros((2, cap.e_cap), dtype=torch.int32), i32(cap.n_cap),
                              i32(cap.e_cap), None, None, i32(B), torch.ones(B, dtype=torch.bool), i32(4), cap, 3)


@pytest.mark.parametrize("K,d", list(itertools.product([1, 2, 5, 64], [1, 32])))
def test_dense_pooled_capacities_against_brute_force(K, d):
    """The largest batch there is — B live slots, every block dense — needs exactly the rows and edges the capacities give, and
    its padded tail fits the sinks with no sink above d edges."""
    for B in (0, 1, 3, 10):
        batch = _static_batch(B, d)
        for drop in (False, True):
            cap = batch.dense_pooled_capacities(K, drop_diagonal=drop)
            rows = sum(K for _ in range(B))
            edges = sum(1 for _ in range(B) for c1 in range(K) for c2 in range(K) if not (drop and c1 == c2))
            assert (cap.batch_size, cap.max_nodes, cap.max_edges, cap.e_cap, cap.sink_degree) == (B, rows, edges, edges, d)
            assert cap.n_cap == rows + cap.sinks and cap.sinks >= 1
            assert cap.sinks * d >= edges and (cap.sinks - 1) * d < max(edges, 1)          # the fewest sinks that hold an empty batch's tail
            assert (cap.max_nodes, cap.max_edges, cap.sinks, cap.n_cap, cap.e_cap) == mirror_dense_capacities(B, K, d, drop)
            # an empty batch pads every edge: sink t holds edges [t d, (t + 1) d)
            m = mirror_dense_pool_static(np.zeros((B * K, K), np.float32), np.zeros(B, bool), [0, 0, 0, 0], K, drop, cap.n_cap,
                                         cap.e_cap, cap.sinks, d)
            assert m["e_live"] == 0 and np.bincount(m["edge_index"][0], minlength=cap.n_cap).max(initial=0) <= d
            assert (m["edge_index"] >= cap.max_nodes).all() and (m["edge_index"] < cap.n_cap).all()


def test_dense_pooled_capacities_refusals():
    batch = _static_batch(4, 32)
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="num_clusters"):
            batch.dense_pooled_capacities(bad)
    big = _static_batch(1 << 20, 32)
    with pytest.raises(ValueError, match="int32"):
        big.dense_pooled_capacities(64)
