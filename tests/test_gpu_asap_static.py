# coding=utf-8
"""ASAP on fixed-shape batches (include/tfgx_asap_static.h, nn/pool/asap_static.py) on the GPU: the three kernels against their
numpy mirrors, exactly; the level's layout against the mirror given the route's own P and selection; two stacked levels against
the float64 ASAP mirror with inert padding; the eager route on a store without self-loops; dropout by position; no host read and
no sort; capture and replay; refusals; composition with the other static pools; the example."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from asap_mirror import WEIGHT_NAMES, asap_mirror, make_weights, topk_select
from asap_static_mirror import mirror_asap_layout, mirror_assignment, mirror_clusters
from densepool_static_mirror import mirror_pooled_weight
from test_collate_abi import random_dataset
from test_gpu_collate import _eq, _plan_eq
from test_gpu_nbrblock import _close

pytestmark = pytest.mark.gpu

DEV = "cuda"
F, A = 5, 4
# a dozen graphs of (nodes, edges): an empty one, one without edges, some with fewer nodes than k = 3 / 64, and a 70-node star
# whose centre row holds 138 duplicated edges and 3 live self-loops (longer than the kernels' 64-edge chunk, absent edges in it)
SIZES = [(0, 0), (1, 1), (2, 3), (3, 5), (7, 12), (33, 70), (40, 90), (6, 0), (12, 30), (25, 60), (17, 40), (70, 215)]
EMPTY, NO_EDGES, STAR = 0, 7, 11
BATCHES = {"dead slots last": [5, EMPTY, NO_EDGES, 2, STAR, 9, 3, -1, -1],
           "dead slots interleaved": [-1, 5, -1, EMPTY, NO_EDGES, 2, -1, STAR, 9, 3, -1],
           "all slots dead": [-1, -1, -1]}
SELECTIONS = [(1, None), (3, None), (64, None), (None, 0.5)]
_WORLD = {}


def _star(n):
    """The centre 0 reads every leaf twice, every leaf reads the centre; 3 self-loops on the centre and 5 on leaves."""
    leaves = np.arange(1, n)
    row = np.concatenate([np.zeros(2 * (n - 1), np.int64), leaves, [0, 0, 0], leaves[:5]])
    col = np.concatenate([leaves, leaves, np.zeros(n - 1, np.int64), [0, 0, 0], leaves[:5]])
    return np.stack([row, col])


def _dataset(seed, loops=True):
    d = random_dataset(np.random.Generator(np.random.PCG64(seed)), SIZES, F, y=False)      # weights uniform in [0.5, 1.5]: positive
    e0 = int(d["edge_ptr"][STAR])
    star = _star(SIZES[STAR][0])
    assert star.shape[1] == SIZES[STAR][1]
    d["edge_index"][:, e0:e0 + star.shape[1]] = star + int(d["node_ptr"][STAR])
    if not loops:                                               # every self-loop becomes an edge to the next node of its graph
        ei = d["edge_index"]
        for g, (n, _) in enumerate(SIZES):
            e0, e1, n0 = int(d["edge_ptr"][g]), int(d["edge_ptr"][g + 1]), int(d["node_ptr"][g])
            same = np.flatnonzero(ei[0, e0:e1] == ei[1, e0:e1]) + e0
            if n > 1:
                ei[1, same] = n0 + (ei[1, same] - n0 + 1) % n
        assert ((ei[0] != ei[1]) | np.isin(np.arange(ei.shape[1]), np.arange(int(d["edge_ptr"][1]), int(d["edge_ptr"][2])))).all()
    d["y"] = (np.arange(len(SIZES), dtype=np.int64) % 3).reshape(-1, 1)
    return d


def _world(loops=True):
    """(GraphStore, its packed arrays): built once and left unchanged.  loops=False: a store without self-loops (the one-node
    graph aside, whose only edge is one, and which the no-loop test leaves out)."""
    if loops not in _WORLD:
        import tf_geometric_amd as tfg
        d = _dataset(277 if loops else 278, loops)
        _WORLD[loops] = (tfg.data.GraphStore.from_arrays(**d), d)
    return _WORLD[loops]


def _ids(ids):
    return torch.tensor(ids, dtype=torch.int32, device=DEV)


def _weights(seed, f=F, grad=False, scale=1.0):
    w = make_weights(np.random.Generator(np.random.PCG64(seed)), f, A, scale=scale)
    return w, [torch.from_numpy(w[n]).to(DEV).requires_grad_(grad) for n in WEIGHT_NAMES]


def _rebuilt(ei, n):
    from tf_geometric_amd.plan import CsrPlan
    ei = ei.clone()
    plan, flip = CsrPlan.build(ei, n, n), CsrPlan.build(torch.stack([ei[1], ei[0]]), n, n)
    return [plan.row_ptr, plan.col, plan.perm], [flip.row_ptr, flip.col, flip.perm]


def _live_batch(store, slots):
    live = [i for i in slots if i >= 0]
    ref = store.collate(live)
    gid = np.repeat([j for j, i in enumerate(slots) if i >= 0], [SIZES[i][0] for i in live])      # the slot number as graph index
    return live, ref, gid


# ---- 1. the kernels against their mirrors ------------------------------------------------------------------------------------------
def _attend_reference(row_ptr, col, x, sq, sh, bias, skip):
    """(c, p, p_self) in float64 from the header's words."""
    n = len(row_ptr) - 1
    c, p, ps = np.zeros((n, x.shape[1])), np.zeros(len(col)), np.zeros(n)
    leaky = lambda z: np.where(z > 0, z, 0.2 * z)      # noqa: E731
    for i in range(n):
        es = [e for e in range(row_ptr[i], row_ptr[i + 1]) if not (skip and col[e] == i)]
        s = np.concatenate([[leaky(sq[i] + sh[i] + bias)], leaky(sq[i] + sh[col[es]] + bias)])
        ex = np.exp(s - s.max())
        w = ex / (ex.sum() + 1e-8)
        ps[i], p[es] = w[0], w[1:]
        c[i] = w[0] * x[i] + (w[1:, None] * x[col[es]]).sum(axis=0)
    return c, p, ps


@pytest.mark.parametrize("sink_degree", [1, 32])
def test_attention_with_absent_edges_and_the_assignment_equal_their_mirrors(tfg, sink_degree):
    from tf_geometric_amd import _lib as L, autograd as AG
    from tf_geometric_amd.plan import CACHE_KEY_PLAN
    from tf_geometric_amd.nn.pool.asap_static import asap_assignment
    from tf_geometric_amd.nn.pool.sag_pool_static import select_static
    store, _ = _world()
    slots = BATCHES["dead slots interleaved"]
    batch = store.collate_static(_ids(slots), store.static_capacities(len(slots), sink_degree=sink_degree))
    cap, B = batch.capacities, len(slots)
    plan = batch.cache[CACHE_KEY_PLAN]
    row_ptr, col = plan.row_ptr.cpu().numpy(), plan.col.cpu().numpy()
    star_row = int(batch.graph_row_ptr[slots.index(STAR)])
    seg = col[row_ptr[star_row]:row_ptr[star_row + 1]]
    assert seg.shape[0] == 141 and (seg == star_row).sum() == 3 and np.unique(seg).shape[0] == 70      # > 64 edges, absent ones, duplicates
    gen = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn((cap.n_cap, F), generator=gen).to(DEV)
    sq, sh = torch.randn(cap.n_cap, generator=gen).to(DEV), torch.randn(cap.n_cap, generator=gen).to(DEV)
    bias = torch.tensor([0.25], device=DEV)
    # (a) skip on: float64 reference; p = 0 exactly on absent edges
    c, p, ps, _, _ = AG.asap_attend_forward(plan, x, sq, sh, bias, skip_self_loops=True)
    rc, rp, rps = _attend_reference(row_ptr, col, x.cpu().numpy().astype(np.float64), sq.cpu().numpy().astype(np.float64),
                                    sh.cpu().numpy().astype(np.float64), 0.25, True)
    _close(c.cpu().numpy(), rc, "attend: c")
    _close(p.cpu().numpy(), rp, "attend: p")
    _close(ps.cpu().numpy(), rps, "attend: p_self")
    rows = np.repeat(np.arange(cap.n_cap), np.diff(row_ptr))
    absent = rows == col
    assert absent.sum() > cap.e_cap - int(batch.counts[2]) and not p.cpu().numpy()[absent].any()
    # skip off is the existing entry, bit for bit (the shared body); so is a device seed with dropout
    lib = L.load_library()
    old = AG.asap_attend_forward(plan, x, sq, sh, bias, 0.5, 12345)
    seed_dev = torch.tensor([12345], dtype=torch.int64, device=DEV)
    new = AG.asap_attend_forward(plan, x, sq, sh, bias, 0.5, seed_dev)
    assert all(torch.equal(a, b) for a, b in zip(old, new))
    # dropout by position under skip: p_drop = p * keep / (1 - rate) at the CSR position, e_cap + i for the self edge
    c2, p2, ps2, pd, pds = AG.asap_attend_forward(plan, x, sq, sh, bias, 0.5, 12345, skip_self_loops=True)
    assert torch.equal(p2, p) and torch.equal(ps2, ps)
    keep = np.asarray([lib.tfgx_dropout_keep(12345, q, 0.5) for q in range(cap.e_cap + cap.n_cap)], np.float32)
    scale = keep * (np.float32(1.0) / (np.float32(1.0) - np.float32(0.5)))
    assert 0.3 < keep.mean() < 0.7
    _eq(pd, p.cpu().numpy() * scale[:cap.e_cap], "p_drop")
    _eq(pds, ps.cpu().numpy() * scale[cap.e_cap:], "p_self_drop")
    # (b) the assignment, exactly: float32 sums in CSR order
    for k, ratio in SELECTIONS:
        K = batch.asap_clusters_per_graph(k=k, ratio=ratio)
        sel = select_static(batch, sq, k, ratio, batch.asap_pooled_capacities(k=k, ratio=ratio), "test")
        S = asap_assignment(plan, pd, pds, sel, B, K)
        m_rows = sel.capacities.max_nodes
        ref = mirror_assignment(row_ptr, col, pd.cpu().numpy(), pds.cpu().numpy(), sel.node_index.cpu().numpy()[:m_rows],
                                sel.node_graph_index.cpu().numpy()[:m_rows], sel.pooled_row_ptr.cpu().numpy(), B, K)
        _eq(S, ref, "S k={} ratio={}".format(k, ratio))
        assert not S[int(batch.counts[1]):].any()                # dead rows of the parent are in no cluster


def test_centred_attention_backward_equals_float64_and_keeps_the_epsilon_gradient(tfg):
    """tfgx_asapstatic_attend_backward_f32 against ds_e = p_e (u_e - sum_j p_j u_j) in float64 on the batch with the star (rows of
    several chunks, absent edges, duplicates), without and with dropout; and on rows of ONE term — every row of the all-dead
    batch has only absent edges — the gradient is p_self dp_self 1e-8 / D, where the uncentred entry returns exactly 0."""
    from tf_geometric_amd import _lib as L, autograd as AG
    from tf_geometric_amd.plan import CACHE_KEY_PLAN
    lib = L.require_gpu()
    store, _ = _world()

    def backward(plan, sq, sh, bias, p, ps, pd, pds, dp, dps, entry):
        N, E = plan.n_dst, plan.num_edges
        ds, dss, dsq = torch.empty(E, device=DEV), torch.empty(N, device=DEV), torch.empty(N, device=DEV)
        args = [L.ptr(plan.row_ptr), L.ptr(plan.col), N, E, L.ptr(sq), L.ptr(sh), L.ptr(bias), L.ptr(p), L.ptr(ps), L.ptr(pd), L.ptr(pds),
                L.ptr(dp), L.ptr(dps)]
        if entry == "centred":
            L.check(lib.tfgx_asapstatic_attend_backward_f32(*args, 1, L.ptr(ds), L.ptr(dss), L.ptr(dsq), L.stream_ptr()), entry)
        else:
            L.check(lib.tfgx_asap_attend_backward_f32(*args, L.ptr(ds), L.ptr(dss), L.ptr(dsq), L.stream_ptr()), entry)
        return ds.cpu().numpy(), dss.cpu().numpy(), dsq.cpu().numpy()

    gen = torch.Generator(device="cpu").manual_seed(13)
    slots = BATCHES["dead slots interleaved"]
    batch = store.collate_static(_ids(slots))
    cap = batch.capacities
    plan = batch.cache[CACHE_KEY_PLAN]
    row_ptr, col = plan.row_ptr.cpu().numpy(), plan.col.cpu().numpy()
    rows = np.repeat(np.arange(cap.n_cap), np.diff(row_ptr))
    x = torch.randn((cap.n_cap, F), generator=gen).to(DEV)
    sq, sh = torch.randn(cap.n_cap, generator=gen).to(DEV), torch.randn(cap.n_cap, generator=gen).to(DEV)
    bias = torch.tensor([0.25], device=DEV)
    dp, dps = torch.randn(cap.e_cap, generator=gen).to(DEV), torch.randn(cap.n_cap, generator=gen).to(DEV)
    sq64, sh64 = sq.cpu().numpy().astype(np.float64), sh.cpu().numpy().astype(np.float64)
    _, p64, ps64 = _attend_reference(row_ptr, col, np.zeros((cap.n_cap, 1)), sq64, sh64, 0.25, True)
    for rate in (0.0, 0.5):
        _, p, ps, pd, pds = AG.asap_attend_forward(plan, x, sq, sh, bias, rate, 777, skip_self_loops=True)
        k_e = np.ones(cap.e_cap) if pd is None else np.asarray([lib.tfgx_dropout_keep(777, q, rate) for q in range(cap.e_cap)]) / (1 - rate)
        k_s = np.ones(cap.n_cap) if pd is None else np.asarray([lib.tfgx_dropout_keep(777, cap.e_cap + q, rate) for q in range(cap.n_cap)]) / (1 - rate)
        u, us = k_e * dp.cpu().numpy().astype(np.float64), k_s * dps.cpu().numpy().astype(np.float64)
        t = np.zeros(cap.n_cap)
        np.add.at(t, rows, p64 * u)
        t += ps64 * us
        slope = lambda z: np.where(z > 0, 1.0, 0.2)      # noqa: E731
        ref_ds = p64 * (u - t[rows]) * slope(sq64[rows] + sh64[col] + 0.25)
        ref_dss = ps64 * (us - t) * slope(sq64 + sh64 + 0.25)
        ref_dsq = ref_dss.copy()
        np.add.at(ref_dsq, rows, ref_ds)
        got = backward(plan, sq, sh, bias, p, ps, pd, pds, dp, dps, "centred")
        for g, r, what in zip(got, (ref_ds, ref_dss, ref_dsq), ("ds", "ds_self", "dsq")):
            _close(g, r, "rate {}: {}".format(rate, what))
        # every entry of a one-term row, not only the tensor's largest: the dead rows have no edge but absent ones
        one_term = np.flatnonzero(np.bincount(rows[rows != col], minlength=cap.n_cap) == 0)
        assert one_term.size > 10
        live_terms = ref_dss[one_term][us[one_term] != 0]
        assert (np.abs(live_terms) > 0).all() and (np.abs(live_terms) < 1e-6).all()
        assert np.abs(got[1][one_term] - ref_dss[one_term]).max() <= 1e-5 * np.abs(ref_dss[one_term]).max()
        old = backward(plan, sq, sh, bias, p, ps, pd, pds, dp, dps, "uncentred")
        assert not old[1][one_term].any()                        # what the centred form is for


def test_a_list_without_self_loops_gives_the_existing_entry_bit_for_bit(tfg):
    from tf_geometric_amd import autograd as AG
    from tf_geometric_amd.plan import CsrPlan
    rng = np.random.Generator(np.random.PCG64(5))
    n = 300
    ei = np.stack([rng.integers(0, n, 4000), rng.integers(0, n, 4000)])
    ei[0, :200] = 7                                              # a row of several chunks
    ei = ei[:, ei[0] != ei[1]].astype(np.int32)
    plan = CsrPlan.build(torch.from_numpy(ei).to(DEV), n, n)
    gen = torch.Generator(device="cpu").manual_seed(6)
    for f in (0, 5, 64, 130, 256):
        x = torch.randn((n, f), generator=gen).to(DEV)
        sq, sh = torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV)
        bias = torch.tensor([-0.1], device=DEV)
        for rate in (0.0, 0.3):
            old = AG.asap_attend_forward(plan, x, sq, sh, bias, rate, 99)
            new = AG.asap_attend_forward(plan, x, sq, sh, bias, rate, 99, skip_self_loops=True)
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(old, new)), (f, rate)


def _raw_edges(P, prp, counts, K, n_cap, e_cap, sinks, d):
    """tfgx_asapstatic_edges on a P given as it is: a dict of its outputs (numpy)."""
    from tf_geometric_amd.nn.pool.asap_static import asap_layout
    from tf_geometric_amd.data.graph_store import StaticBatchCapacities
    B = len(prp) - 2
    cap = StaticBatchCapacities(B, n_cap - sinks, e_cap, d, sinks, n_cap, e_cap)
    Pt = None if K == 0 else torch.from_numpy(np.ascontiguousarray(P, np.float32)).to(DEV)
    ct = torch.tensor(counts, dtype=torch.int32, device=DEV)
    ei, src, egi, plans = asap_layout(Pt, torch.tensor(prp, dtype=torch.int32, device=DEV), ct, K, cap)
    return dict(edge_index=ei, edge_src=src, edge_graph_index=egi, counts=ct, plan=plans[0], plan_t=plans[1])


@pytest.mark.parametrize("sink_degree", [1, 32])
@pytest.mark.parametrize("K", [0, 1, 3, 35, 64])
def test_edges_kernel_on_signed_zeros_and_nans_equals_the_mirror(tfg, K, sink_degree):
    """Every output of the launch sequence on a P with -0.0 (no edge) and NaN (an edge), ragged slots, empty and full ones."""
    rng = np.random.Generator(np.random.PCG64(K * 2 + sink_degree))
    for B in (7, 1):
        P = rng.integers(1, 4, (B * K, K)).astype(np.float32) * (rng.random((B * K, K)) < 0.5)
        flat = P.reshape(-1)
        if flat.size >= 9:
            flat[rng.integers(0, flat.size, flat.size // 9)] = np.nan
            flat[rng.integers(0, flat.size, flat.size // 9)] = -0.0
        m = rng.integers(0, K + 1, B)
        m[0] = K
        if B > 2:
            m[2] = 0
        prp = np.concatenate([[0], np.cumsum(m)])
        m_max = int(prp[-1]) + 5
        e_cap = K * m_max
        sinks = max(1, -(-e_cap // sink_degree))
        n_cap = m_max + sinks
        prp = np.concatenate([prp, [n_cap]])
        got = _raw_edges(P, prp, [B, prp[B], -7, 2], K, n_cap, e_cap, sinks, sink_degree)
        ref = mirror_asap_layout(P, prp, [B, prp[B], -7, 2], K, n_cap, e_cap, sinks, sink_degree)
        for key in ("edge_index", "edge_src", "edge_graph_index", "counts"):
            _eq(got[key], ref[key], "K={} B={}: {}".format(K, B, key))
        _plan_eq(got["plan"], ref["plan"], "by row")
        _plan_eq(got["plan_t"], ref["plan_t"], "by column")


# ---- 2. the level: layout, selection, plans ----------------------------------------------------------------------------------------
def _check_level(tfg, pooled, parent, k, ratio, what):
    from tf_geometric_amd.plan import CACHE_KEY_PLAN, attached_plan
    from tf_geometric_amd.nn.pool.common_pool import CACHE_KEY_GRAPH_PLAN, _graph_plan
    B, cap = parent.num_slots, pooled.capacities
    K = parent.asap_clusters_per_graph(k=k, ratio=ratio)
    assert cap == parent.asap_pooled_capacities(k=k, ratio=ratio) and isinstance(pooled, tfg.data.StaticBatchGraph)
    assert (pooled.num_nodes, pooled.num_edges, pooled.num_graphs) == (cap.n_cap, cap.e_cap, B + 1)
    assert pooled.max_degree() == pooled.max_graph_nodes() == K
    # the selection is topk_pool's on the route's own float32 scores, exactly
    n_live, m_live = int(parent.counts[1]), int(pooled.counts[1])
    gid = parent.node_graph_index.cpu().numpy()[:n_live]
    score = pooled.node_score.cpu().numpy()
    assert score.dtype == np.float32 and score.shape == (parent.capacities.n_cap,)
    want = topk_select(gid, score[:n_live], k, ratio) if n_live else np.zeros(0, np.int64)
    node_index = pooled.node_index.cpu().numpy()
    assert np.array_equal(node_index[:m_live], want) and (node_index[m_live:] == -1).all(), what + ": selection"
    ngi = pooled.node_graph_index.cpu().numpy()
    assert np.array_equal(ngi[:m_live], gid[want]) and (ngi[m_live:] == B).all()
    prp = pooled.graph_row_ptr.cpu().numpy()
    assert np.array_equal(prp[:B + 1], np.concatenate([[0], np.cumsum(np.bincount(ngi[:m_live], minlength=B))])) and prp[B + 1] == cap.n_cap
    # the layout is the mirror's, given the route's own P
    P = None if K == 0 else pooled.asap_blocks.cpu().numpy()
    counts = pooled.counts.cpu().numpy()
    m = mirror_asap_layout(P, prp, counts, K, cap.n_cap, cap.e_cap, cap.sinks, cap.sink_degree)
    for key in ("edge_index", "edge_graph_index", "edge_src", "counts"):
        _eq(getattr(pooled, key), m[key], "{}: {}".format(what, key))
    assert list(counts[:2]) == [int(parent.counts[0]), m_live] and counts[3] == int(parent.counts[3])
    _eq(pooled.edge_weight, mirror_pooled_weight(P if K else np.zeros(0, np.float32), m["edge_src"]), what + ": edge_weight")
    assert not pooled.edge_weight.requires_grad
    assert pooled.y is parent.y and pooled.ids is parent.ids and pooled.graph_mask is parent.graph_mask
    assert pooled.check() is pooled
    plan = attached_plan(pooled.edge_index)
    assert plan is not None and plan is pooled.cache[CACHE_KEY_PLAN] and plan._transposed._transposed is plan
    _plan_eq(plan, m["plan"], what + ": by row")
    _plan_eq(plan._transposed, m["plan_t"], what + ": by column")
    rebuilt, flip = _rebuilt(pooled.edge_index, cap.n_cap)
    _plan_eq(plan, rebuilt, what + ": rebuilt")
    _plan_eq(plan._transposed, flip, what + ": rebuilt flip")
    g_ngi, version, graph_plan = pooled.cache[CACHE_KEY_GRAPH_PLAN]
    assert g_ngi is pooled.node_graph_index and version == g_ngi._version
    fresh = _graph_plan(g_ngi.clone(), B + 1, cap.n_cap, None)
    _plan_eq(graph_plan, [fresh.row_ptr, fresh.col, fresh.perm], what + ": graph plan")
    assert not pooled.x.detach()[m_live:].any(), what + ": dead rows of pooled x"
    return m


@pytest.mark.parametrize("sink_degree", [1, 32])
@pytest.mark.parametrize("k,ratio", SELECTIONS + [(0, None)])
def test_level_layout_selection_and_plans(tfg, k, ratio, sink_degree):
    store, _ = _world()
    _, w1 = _weights(1)
    _, w2 = _weights(2)
    for name, slots in BATCHES.items():
        batch = store.collate_static(_ids(slots), store.static_capacities(len(slots), sink_degree=sink_degree))
        with torch.no_grad():
            one = tfg.nn.asap_static(batch.x, batch, *w1, k=k, ratio=ratio)
            two = tfg.nn.asap_static(one.x, one, *w2, k=k, ratio=ratio)      # meets one live unit self-loop per cluster
        what = "k={} ratio={} d={} {}".format(k, ratio, sink_degree, name)
        m1 = _check_level(tfg, one, batch, k, ratio, what + " level 1")
        m2 = _check_level(tfg, two, one, k, ratio, what + " level 2")
        live = [i for i in slots if i >= 0]
        want = sum(mirror_clusters(SIZES[i][0], k, ratio) for i in live)
        assert m1["m_live"] == want and m2["m_live"] == sum(
            mirror_clusters(mirror_clusters(SIZES[i][0], k, ratio), k, ratio) for i in live)
        assert m1["e_live"] >= m1["m_live"] and two.capacities.e_cap <= one.capacities.e_cap      # the capacities shrink
        if k == 0:
            assert one.capacities.e_cap == 0 and one.asap_blocks is None and m1["m_live"] == 0 and int(one.counts[0]) == len(live)
        for j, i in enumerate(slots):
            if i == NO_EDGES and k != 0:                         # a graph without edges keeps its clusters, each with its self-loop alone
                mine = m1["edge_graph_index"] == j
                assert mine.sum() == mirror_clusters(SIZES[i][0], k, ratio) and (m1["edge_src"][mine] == -1).all()
            if i == EMPTY:
                assert not (m1["edge_graph_index"] == j).any()


# ---- 3. two stacked levels against float64 -----------------------------------------------------------------------------------------
def _two_levels(tfg, batch, x, ws, k, ratio, **kw):
    one = tfg.nn.asap_static(x, batch, *ws[0], k=k, ratio=ratio, **kw)
    two = tfg.nn.asap_static(one.x, one, *ws[1], k=k, ratio=ratio, **kw)
    return one, two


def _objective(levels, R):
    """A fixed linear functional of both levels' pooled x (R: one random row vector per level)."""
    return sum((lv.x * r).sum() for lv, r in zip(levels, R))


_RUNS = {}
# (seed, scale) of the two levels' weights.  Level 2 sees at most k nodes per graph; a softmax over so few scores that lie on one
# side of leaky_relu's kink does not feel a shift of them, and the gradients of the attention biases and of everything in front
# of the per-row half of the score then consist of the denominator's 1e-8 alone.  This pair was chosen ON THE FLOAT64 MIRROR (no
# GPU) so that for k = 3, k = 64 and ratio = 0.5 every one of the 22 reference gradients has an entry above 1e-3; the gradient
# test asserts that.  At k = 1 no weights can do it (every level-2 graph is one node): see its docstring.
LEVEL_WEIGHTS = ((11, 1.0), (15, 2.0))


def _level_weights():
    return [_weights(seed, grad=True, scale=scale)[1] for seed, scale in LEVEL_WEIGHTS]


def _two_level_runs(tfg, k, ratio):
    """Both levels on "dead slots last" and "dead slots interleaved", each with clean and with NaN dead rows of x, backward through
    a fixed linear functional; and the float64 mirror on the live graphs, given the route's own selection.  Computed once per
    (k, ratio), shared by the three tests below and left unchanged."""
    if (k, ratio) in _RUNS:
        return _RUNS[(k, ratio)]
    store, d = _world()
    np_w = [_weights(*LEVEL_WEIGHTS[0][:1], scale=LEVEL_WEIGHTS[0][1])[0], _weights(*LEVEL_WEIGHTS[1][:1], scale=LEVEL_WEIGHTS[1][1])[0]]
    gen = torch.Generator(device="cpu").manual_seed(8)
    R = [torch.randn(F, generator=gen).to(DEV), torch.randn(F, generator=gen).to(DEV)]
    out = {"R": R}
    for name in ("dead slots last", "dead slots interleaved"):
        slots = BATCHES[name]
        live, cb, gid = _live_batch(store, slots)
        batch = store.collate_static(_ids(slots))
        n_live = cb.num_nodes
        for garbage in (False, True):
            ws = _level_weights()
            x = batch.x.clone()
            if garbage:
                x[n_live:] = float("nan")
            x.requires_grad_(True)
            one, two = _two_levels(tfg, batch, x, ws, k, ratio)
            _objective((one, two), R).backward()
            out[(name, garbage)] = (one, two, x.grad, [w.grad for lv in ws for w in lv], n_live)
    one, two = out[("dead slots last", False)][:2]
    m1, m2 = int(one.counts[1]), int(two.counts[1])
    idx1, idx2 = one.node_index[:m1].cpu().numpy(), two.node_index[:m2].cpu().numpy()
    leaves = [{n: torch.from_numpy(w[n]).double().requires_grad_(True) for n in WEIGHT_NAMES} for w in np_w]
    x64 = cb.x.cpu().double().requires_grad_(True)
    r1 = asap_mirror(x64, cb.edge_index.cpu().numpy(), cb.edge_weight.cpu().numpy(), gid, leaves[0], k=k, ratio=ratio, topk_node_index=idx1)
    r2 = asap_mirror(r1["x"], r1["edge_index"], r1["edge_weight"].numpy(), r1["node_graph_index"], leaves[1], k=k, ratio=ratio,
                     topk_node_index=idx2)
    ((r1["x"] * R[0].cpu().double()).sum() + (r2["x"] * R[1].cpu().double()).sum()).backward()
    out["ref"] = (r1, r2, x64.grad.numpy(), [leaves[lv][n].grad.numpy() for lv in range(2) for n in WEIGHT_NAMES], idx1, idx2)
    _RUNS[(k, ratio)] = out
    return out


GRAD_NAMES = ["level {} {}".format(lv + 1, n) for lv in range(2) for n in WEIGHT_NAMES]


@pytest.mark.parametrize("k,ratio", SELECTIONS)
def test_two_levels_equal_the_float64_mirror(tfg, k, ratio):
    """Live x, the live edge list and the pooled weights of both levels against tests/asap_mirror.py in float64 (every entry
    within 1e-5 of the tensor's largest reference magnitude), the mirror given the route's own selection — which is the same for
    dead slots last and interleaved."""
    runs = _two_level_runs(tfg, k, ratio)
    r1, r2, _, _, ridx1, ridx2 = runs["ref"]
    for name in ("dead slots last", "dead slots interleaved"):
        one, two = runs[(name, False)][:2]
        m1, m2 = int(one.counts[1]), int(two.counts[1])
        assert np.array_equal(one.node_index[:m1].cpu().numpy(), ridx1) and np.array_equal(two.node_index[:m2].cpu().numpy(), ridx2), \
            name + ": another selection than the first batch's"
        for lv, r, m_lv, what in ((one, r1, m1, "level 1"), (two, r2, m2, "level 2")):
            _close(lv.x.detach()[:m_lv].cpu().numpy(), r["x"].detach().numpy(), "{} {}: x".format(name, what))
            e = int(lv.counts[2])
            order = np.argsort(r["edge_index"][0], kind="stable")
            assert np.array_equal(lv.edge_index[:, :e].cpu().numpy(), r["edge_index"][:, order]), "{} {}: edge list".format(name, what)
            _close(lv.edge_weight[:e].cpu().numpy(), r["edge_weight"].numpy()[order], "{} {}: edge weights".format(name, what))
            assert int((lv.edge_index[0, :e] == lv.edge_index[1, :e]).sum()) == m_lv          # one live unit self-loop per cluster


@pytest.mark.parametrize("k,ratio", SELECTIONS)
def test_two_levels_gradients_equal_float64_autograd(tfg, k, ratio):
    """d/dx and the gradients of the eleven weights of both levels against float64 autograd on the mirror: every entry within 1e-5
    of the tensor's largest reference magnitude.  Every tensor is compared and printed before anything is asserted.

    At k = 1 every graph of level 2 is ONE node whose only edge is its absent self-loop: its softmax has one term,
    p_self = 1 / (1 + 1e-8), and the gradients of the six level-2 attention weights consist of the denominator's epsilon alone
    (largest reference entries 2.7e-8 to 1.6e-7).  The centred backward (tfgx_asapstatic_attend_backward_f32) keeps them; three
    LEConv gradients of that level are exactly 0 in both (a graph of one node has no edge), which the bar demands exactly."""
    runs = _two_level_runs(tfg, k, ratio)
    _, _, rgx, rgw, _, _ = runs["ref"]
    smallest = min(float(np.abs(r).max()) for r in rgw)
    print("float64 reference: the smallest of the 22 gradients' largest |entry| = {:.3e}".format(smallest))
    if k != 1:
        assert smallest > 1e-3, "a reference gradient consists of the softmax's epsilon alone: choose other weights"
    missed = []

    def close(got, ref, what):
        """_close's bar without its demand for a non-zero reference: a gradient that is exactly 0 must come out exactly 0."""
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        assert got.shape == ref.shape, what
        scale, err = float(np.abs(ref).max()), float(np.abs(got - ref).max())
        print("{:<60s} max|err| = {:.3e}   bar = {:.3e}".format(what, err, 1e-5 * scale))
        if not err <= 1e-5 * scale:
            missed.append("{}: max|err| {:.3e} > 1e-5 * {:.3e}".format(what, err, scale))

    for name in ("dead slots last", "dead slots interleaved"):
        _, _, gx, gw, n_live = runs[(name, False)]
        close(gx[:n_live].cpu().numpy(), rgx, name + ": d/dx")
        for g, r, what in zip(gw, rgw, GRAD_NAMES):
            assert g is not None and torch.isfinite(g).all(), what
            close(g.cpu().numpy().reshape(r.shape), r, "{}: d/d {}".format(name, what))
    assert not missed, "\n".join(missed)


@pytest.mark.parametrize("k,ratio", SELECTIONS)
def test_padding_is_inert(tfg, k, ratio):
    """NaN in the dead rows of x: every live output bit and every gradient bit stays, dead rows of x get a zero gradient.  A batch
    without a live slot keeps nothing and has finite gradients."""
    runs = _two_level_runs(tfg, k, ratio)
    for name in ("dead slots last", "dead slots interleaved"):
        (one, two, gx, gw, n_live), (one_g, two_g, gx_g, gw_g, _) = runs[(name, False)], runs[(name, True)]
        for a, b, parent_live in ((one, one_g, n_live), (two, two_g, int(one.counts[1]))):
            for key in ("x", "edge_index", "edge_weight", "node_index", "counts", "node_score"):
                ta, tb = getattr(a, key).detach(), getattr(b, key).detach()
                if key == "node_score":                          # the scores of dead rows are nobody's
                    ta, tb = ta[:parent_live], tb[:parent_live]
                assert torch.equal(ta, tb), "{}: garbage in the dead rows of x changed {}".format(name, key)
        assert torch.equal(gx[:n_live], gx_g[:n_live]) and not gx[n_live:].any() and not gx_g[n_live:].any()
        assert all(torch.equal(a, b) for a, b in zip(gw, gw_g)), name + ": garbage changed a weight gradient"
    store, _ = _world()
    dead = store.collate_static(_ids(BATCHES["all slots dead"]))
    ws = _level_weights()
    x = torch.full_like(dead.x, float("nan")).requires_grad_(True)
    one, two = _two_levels(tfg, dead, x, ws, k, ratio)
    _objective((one, two), runs["R"]).backward()
    assert one.counts.tolist()[:3] == [0, 0, 0] and two.counts.tolist()[:3] == [0, 0, 0] and not one.x.any() and not two.x.any()
    assert not x.grad.any() and all(w.grad is None or torch.isfinite(w.grad).all() for lv in ws for w in lv)


# ---- 4. the eager route on a store without self-loops ------------------------------------------------------------------------------
@pytest.mark.parametrize("k,ratio", SELECTIONS)
def test_live_part_equals_the_eager_route_without_self_loops(tfg, k, ratio):
    store, _ = _world(loops=False)
    _, ws = _weights(21)
    slots = [5, -1, EMPTY, NO_EDGES, STAR, 9, -1, 3, 2]
    live, cb, gid = _live_batch(store, slots)
    assert bool((cb.edge_index[0] != cb.edge_index[1]).all())
    batch = store.collate_static(_ids(slots))
    with torch.no_grad():
        pooled = tfg.nn.asap_static(batch.x, batch, *ws, k=k, ratio=ratio)
        ex, eei, ew, engi = tfg.nn.asap(cb.x, cb.edge_index, cb.edge_weight, torch.from_numpy(gid.astype(np.int32)).to(DEV), *ws, None,
                                        k=k, ratio=ratio)
    m, e = int(pooled.counts[1]), int(pooled.counts[2])
    # nn.asap keeps ITS graph order: np.unique of the slot numbers, which is the slot order
    assert m == int(ex.shape[0]) and e == int(eei.shape[1])
    # node_index first: nn.topk_pool returns parent rows of the collated batch, which are the static batch's live rows
    assert torch.equal(pooled.node_index[:m].long(), torch.from_numpy(topk_select(gid, pooled.node_score[:cb.num_nodes].cpu().numpy(), k, ratio)).to(DEV))
    assert torch.equal(pooled.x[:m], ex), "pooled x differs from nn.asap"
    assert torch.equal(pooled.node_graph_index[:m], engi)
    order = torch.argsort(eei[0].long(), stable=True)
    assert torch.equal(pooled.edge_index[:, :e], eei[:, order]), "edge list"
    _close(pooled.edge_weight[:e].cpu().numpy(), ew[order].cpu().numpy(), "edge weights")


# ---- 5. dropout --------------------------------------------------------------------------------------------------------------------
def test_dropout_follows_the_keep_rule_at_the_csr_positions(tfg):
    from tf_geometric_amd import _lib as L
    from tf_geometric_amd.plan import CACHE_KEY_PLAN
    store, _ = _world()
    lib = L.load_library()
    np_w, ws = _weights(31)
    slots = BATCHES["dead slots interleaved"]
    live, cb, gid = _live_batch(store, slots)
    batch = store.collate_static(_ids(slots))
    cap = batch.capacities
    seed, rate = 2024, 0.4
    with torch.no_grad():
        pooled = tfg.nn.asap_static(batch.x, batch, *ws, k=3, drop_rate=rate, training=True, seed=seed)
        again = tfg.nn.asap_static(batch.x, batch, *ws, k=3, drop_rate=rate, training=True, seed=seed)
        other = tfg.nn.asap_static(batch.x, batch, *ws, k=3, drop_rate=rate, training=True, seed=seed + 1)
        off = tfg.nn.asap_static(batch.x, batch, *ws, k=3, drop_rate=rate, training=False, seed=seed)
        plain = tfg.nn.asap_static(batch.x, batch, *ws, k=3)
    assert torch.equal(pooled.x, again.x) and not torch.equal(pooled.x, other.x) and torch.equal(off.x, plain.x)
    # the host restatement: edge j of collate(live) is edge j of the static batch; its position is where the batch's plan puts it
    perm = batch.cache[CACHE_KEY_PLAN].perm.cpu().numpy()
    position = np.empty(cap.e_cap, np.int64)
    position[perm] = np.arange(cap.e_cap)
    ei = cb.edge_index.cpu().numpy()
    kept_edges = np.flatnonzero(ei[0] != ei[1])
    at = np.concatenate([position[kept_edges], cap.e_cap + np.arange(cb.num_nodes)])
    scale = np.asarray([lib.tfgx_dropout_keep(seed, int(q), rate) for q in at], np.float64) / (1.0 - rate)
    assert 0.4 < (scale > 0).mean() < 0.8
    m = int(pooled.counts[1])
    ref = asap_mirror(cb.x.cpu().numpy(), ei, cb.edge_weight.cpu().numpy(), gid, np_w, k=3, topk_node_index=pooled.node_index[:m].cpu().numpy(),
                      keep_scale=lambda pos: torch.from_numpy(scale))
    _close(pooled.x[:m].cpu().numpy(), ref["x"].numpy(), "pooled x under dropout")
    e = int(pooled.counts[2])
    order = np.argsort(ref["edge_index"][0], kind="stable")
    assert np.array_equal(pooled.edge_index[:, :e].cpu().numpy(), ref["edge_index"][:, order])      # a dropped weight removes its entries
    _close(pooled.edge_weight[:e].cpu().numpy(), ref["edge_weight"].numpy()[order], "pooled weights under dropout")


def _asap_model(tfg, drop_rate, seed=41):
    """GCN(8, relu) -> ASAP(k 3) -> GCN(8, relu) on the pooled batch (so that the pooled edges, weights and plans matter) ->
    mean || max readout -> dense(3), with its parameters."""
    gcn = tfg.layers.GCN(8, activation=tfg.relu, seed=seed)
    gcn._maybe_build([torch.empty(1, F)])
    gcn2 = tfg.layers.GCN(8, activation=tfg.relu, seed=seed + 3)
    gcn2._maybe_build([torch.empty(1, 8)])
    asap = tfg.layers.ASAP(k=3, drop_rate=drop_rate, attention_units=A, seed=seed + 1)
    asap._maybe_build([torch.empty(1, 8)])
    for layer in (gcn, asap, gcn2):
        layer.trainable(True)
    gen = torch.Generator(device="cpu").manual_seed(seed + 2)
    dense = ((torch.rand((16, 3), generator=gen) - 0.5).to(DEV).requires_grad_(True), torch.zeros(3, device=DEV, requires_grad=True))

    def loss(batch, levels=None):
        from tf_geometric_amd import autograd as AG
        h = gcn([batch.x, batch.edge_index, batch.edge_weight], cache=batch.cache, training=True)
        pooled = asap.pool_static(h, batch, training=True)
        if levels is not None:
            levels.append(pooled)
        h2 = gcn2([pooled.x, pooled.edge_index, pooled.edge_weight], cache=pooled.cache, training=True)
        logits = AG.linear(torch.cat([pooled.readout(h2, "mean"), pooled.readout(h2, "max")], dim=-1), *dense)
        per_slot = torch.nn.functional.cross_entropy(logits, batch.y.reshape(-1), reduction="none")
        return torch.where(batch.graph_mask, per_slot, torch.zeros((), device=DEV)).sum() / batch.counts[0].clamp(min=1)

    return gcn.parameters() + asap.parameters() + gcn2.parameters() + list(dense), loss


def test_two_replays_of_a_captured_step_draw_different_masks(tfg):
    """The same batch, a learning rate of 0: the replayed losses differ by the dropout masks alone — and do not differ without
    dropout."""
    store, _ = _world()
    ids = _ids([5, 9, STAR, -1])
    cap = store.static_capacities(4)
    for rate, differ in ((0.5, True), (0.0, False)):
        params, loss = _asap_model(tfg, rate)
        assert len(params) == 2 + 11 + 2 + 2
        opt = torch.optim.Adam(params, lr=0.0, capturable=True)
        step = tfg.CapturedTrainStep(lambda: loss(store.collate_static(ids, cap)), opt)
        losses = [float(step().detach()) for _ in range(3)]
        print("drop_rate", rate, "replayed losses", losses)
        assert np.isfinite(losses).all() and (len(set(losses)) == 3) == differ, losses


# ---- 6. no host read, no sort; capture ---------------------------------------------------------------------------------------------
def _train_store():
    if "train" not in _WORLD:
        import tf_geometric_amd as tfg
        d = _dataset(279)
        _WORLD["train"] = tfg.data.GraphStore.from_arrays(**d)
    return _WORLD["train"]


@pytest.mark.parametrize("rate", [0.0, 0.3])
def test_ids_to_backward_makes_no_host_read_and_no_sort(tfg, monkeypatch, rate):
    from tf_geometric_amd.plan import CsrPlan
    store = _train_store()
    loader = store.static_loader(4, shuffle=True, seed=3)
    cap = store.static_capacities(4)
    params, loss_fn = _asap_model(tfg, rate)

    def step():
        for p in params:
            p.grad = None
        levels = []
        loss = loss_fn(store.collate_static(loader.next_ids(), cap), levels)
        loss.backward()
        return levels, loss

    step()                                                      # the warm call

    def no_build(*a, **k):
        raise AssertionError("a plan was built by sorting")

    monkeypatch.setattr(CsrPlan, "build", staticmethod(no_build))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        levels, loss = step()
        for b in levels:
            for op in ("mean", "sum", "max", "min"):
                b.readout(b.x.detach(), op)
            b.asap_pooled_capacities(ratio=0.5)
            b.pooled_capacities(ratio=0.5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
    assert all(b.check() is b for b in levels)


def test_eager_asap_still_refuses_a_capture(tfg, monkeypatch):
    store, _ = _world()
    b = store.collate([5, 3])
    _, ws = _weights(1)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="asap cannot run inside a hipGraph capture"):
        tfg.nn.asap(b.x, b.edge_index, b.edge_weight, b.node_graph_index, *ws, None, k=3)


def test_pool_static_trains_under_a_capture_as_the_eager_step_does(tfg):
    store = _train_store()
    cap = store.static_capacities(4)

    def world():
        params, loss = _asap_model(tfg, 0.0, seed=51)
        opt = torch.optim.Adam(params, lr=5e-3, capturable=True)
        loader = store.static_loader(4, shuffle=True, seed=13)
        return params, opt, loader, lambda: loss(store.collate_static(loader.next_ids(), cap))

    params, opt, loader, loss_fn = world()
    before = [p.detach().clone() for p in params]
    step = tfg.CapturedTrainStep(loss_fn, opt)
    loader.cursor.zero_()                                       # the warm-up steps advanced it; the weights were rolled back
    captured = [float(step().detach()) for _ in range(3)]
    assert all(not torch.equal(a, b) for a, b in zip(before, params)), "a parameter was not trained"
    params_e, opt_e, loader_e, loss_fn_e = world()
    eager = []
    for _ in range(3):
        opt_e.zero_grad(set_to_none=True)
        loss = loss_fn_e()
        loss.backward()
        opt_e.step()
        eager.append(float(loss.detach()))
    print("eager    ", eager)
    print("captured ", captured, " bit-equal:", captured == eager)
    assert len(set(captured)) == 3                              # every replay trained on another batch, with other weights
    for c, e in zip(captured, eager):
        assert abs(c - e) <= 1e-6 * abs(e), (captured, eager)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_argument(tfg):
    from tf_geometric_amd.data.graph_store import StaticBatchCapacities
    store, _ = _world()
    _, ws = _weights(1)

    def fresh():
        return store.collate_static(_ids([5, 3, -1, 4]))

    batch = fresh()
    n_cap = batch.capacities.n_cap
    with pytest.raises(ValueError, match=r"asap_static: K_blk = 65 .*TFGX_SEGGRAM_MAX_K = 64"):
        tfg.nn.asap_static(batch.x, batch, *ws, k=65)                       # the store's largest graph has 70 nodes
    with pytest.raises(ValueError, match=r"asap_static: K_blk = 70 .*TFGX_SEGGRAM_MAX_K = 64"):
        tfg.nn.asap_static(batch.x, batch, *ws, ratio=1.0)
    tracked = fresh()
    tracked.edge_weight = tracked.edge_weight.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="asap_static: edge_weight requires grad"):
        tfg.nn.asap_static(tracked.x, tracked, *ws, k=3)
    plain = store.collate([5, 3])
    with pytest.raises(ValueError, match="asap_static: batch must be a StaticBatchGraph"):
        tfg.nn.asap_static(plain.x, plain, *ws, k=3)
    good = batch.asap_pooled_capacities(k=3)
    for wrong in (batch.pooled_capacities(k=3), batch.asap_pooled_capacities(k=2),
                  StaticBatchCapacities(*(tuple(good[:2]) + (good.max_edges - 1,) + tuple(good[3:6]) + (good.e_cap - 1,)))):
        with pytest.raises(ValueError, match="asap_static: capacities .* are not batch.asap_pooled_capacities"):
            tfg.nn.asap_static(batch.x, batch, *ws, k=3, capacities=wrong)
    assert tfg.nn.asap_static(batch.x, batch, *ws, k=3, capacities=good).capacities == good
    for kw in (dict(), dict(k=3, ratio=0.5)):
        with pytest.raises(ValueError, match="either k or ratio"):
            tfg.nn.asap_static(batch.x, batch, *ws, **kw)
    with pytest.raises(ValueError, match=r"asap_static: x must have one row per row of the batch \(\[{}, F\]\)".format(n_cap)):
        tfg.nn.asap_static(batch.x[:-1], batch, *ws, k=3)
    lost = fresh()
    lost.cache.clear()
    lost.edge_index = lost.edge_index.clone()
    with pytest.raises(ValueError, match="asap_static: the batch has lost the plans"):
        tfg.nn.asap_static(lost.x, lost, *ws, k=3)
    other = fresh()
    other.capacities = StaticBatchCapacities(*((other.capacities.batch_size, other.capacities.max_nodes + 1) +
                                               tuple(other.capacities[2:5]) + (n_cap + 1, other.capacities.e_cap)))
    with pytest.raises(ValueError, match="asap_static: capacities .* do not describe the batch"):
        tfg.nn.asap_static(torch.zeros((n_cap + 1, F), device=DEV), other, *ws, k=3)
    wide = _weights(1, f=257)[1]
    with pytest.raises(ValueError, match="TFGX_ASAP_MAX_FEATURES"):
        tfg.nn.asap_static(torch.zeros((n_cap, 257), device=DEV), batch, *wide, k=3)


# ---- 8. composition ----------------------------------------------------------------------------------------------------------------
def test_asap_static_composes_with_the_other_static_pools(tfg):
    store, _ = _world()
    np_w, ws = _weights(61)
    slots = [5, -1, 3, NO_EDGES, 9, -1, EMPTY, STAR]
    batch = store.collate_static(_ids(slots), store.static_capacities(len(slots), sink_degree=7))
    gen = torch.Generator(device="cpu").manual_seed(4)

    def against_the_mirror(parent, x, pooled, k, what):
        """The level's live x against the float64 mirror on the parent's live graph (its self-loops stripped by the mirror)."""
        n, e, m = int(parent.counts[1]), int(parent.counts[2]), int(pooled.counts[1])
        ref = asap_mirror(x.detach()[:n].cpu().numpy(), parent.edge_index[:, :e].cpu().numpy(), parent.edge_weight.detach()[:e].cpu().numpy(),
                          parent.node_graph_index[:n].cpu().numpy(), np_w, k=k, topk_node_index=pooled.node_index[:m].cpu().numpy())
        _close(pooled.x.detach()[:m].cpu().numpy(), ref["x"].numpy(), what + ": x")
        order = np.argsort(ref["edge_index"][0], kind="stable")
        ee = int(pooled.counts[2])
        assert np.array_equal(pooled.edge_index[:, :ee].cpu().numpy(), ref["edge_index"][:, order]), what + ": edge list"
        rebuilt, flip = _rebuilt(pooled.edge_index, pooled.capacities.n_cap)
        _plan_eq(pooled.cache["tfgx_csr_plan"], rebuilt, what + ": rebuilt")
        _plan_eq(pooled.cache["tfgx_csr_plan"]._transposed, flip, what + ": rebuilt flip")
        assert pooled.check() is pooled

    with torch.no_grad():
        # (a) after sag_pool_static: the node bound is still the store's
        score = (torch.round(torch.randn(batch.capacities.n_cap, generator=gen) * 2.0) / 2.0).to(DEV).reshape(-1, 1)
        sag = tfg.nn.sag_pool_static(batch.x, batch, lambda inputs, training=None, cache=None: score, ratio=0.5)
        assert sag.max_graph_nodes() == 70
        a = tfg.nn.asap_static(sag.x, sag, *ws, k=4)
        assert a.capacities == sag.asap_pooled_capacities(k=4) and a.max_graph_nodes() == 4
        against_the_mirror(sag, sag.x, a, 4, "asap of sag")
        # (b) after diff_pool_static's coarsening: K = 5 nodes per graph, so K_blk = min(k, 5)
        S = torch.softmax(torch.randn((batch.capacities.n_cap, 5), generator=gen), dim=-1).to(DEV)
        dense = tfg.nn.diff_pool_coarsen_static(batch.x, batch, S)
        assert dense.max_graph_nodes() == 5
        b = tfg.nn.asap_static(dense.x, dense, *ws, k=7)
        assert b.max_graph_nodes() == 5 and b.capacities.max_edges == 5 * b.capacities.max_nodes
        against_the_mirror(dense, dense.x, b, 7, "asap of diff")
        # (c) sag_pool_static after asap_static, against pool_graph on the live pooled graph
        from tf_geometric_amd.utils.subgraph import pool_graph
        one = tfg.nn.asap_static(batch.x, batch, *ws, k=6)
        score2 = (torch.round(torch.randn(one.capacities.n_cap, generator=gen) * 2.0) / 2.0).to(DEV).reshape(-1, 1)
        c = tfg.nn.sag_pool_static(one.x, one, lambda inputs, training=None, cache=None: score2, ratio=0.5, score_activation=torch.tanh)
        m1, e1, m2, e2 = int(one.counts[1]), int(one.counts[2]), int(c.counts[1]), int(c.counts[2])
        assert c.max_degree() == c.max_graph_nodes() == 6 and c.check() is c
        idx = c.node_index[:m2].contiguous()
        px, pei, pw, pgi = pool_graph(one.x[:m1].contiguous(), one.edge_index[:, :e1].contiguous(), one.edge_weight[:e1].contiguous(),
                                      one.node_graph_index[:m1].contiguous(), idx, m1, score=torch.tanh(score2).reshape(-1)[:m1])
        assert int(pei.shape[1]) == e2 and torch.equal(c.x[:m2], px) and torch.equal(c.edge_index[:, :e2], pei)
        assert torch.equal(c.edge_weight[:e2], pw) and torch.equal(c.node_graph_index[:m2], pgi) and not c.x[m2:].any()
        rebuilt, flip = _rebuilt(c.edge_index, c.capacities.n_cap)
        _plan_eq(c.cache["tfgx_csr_plan"], rebuilt, "sag of asap: rebuilt")
        _plan_eq(c.cache["tfgx_csr_plan"]._transposed, flip, "sag of asap: rebuilt flip")
    tracked = tfg.nn.diff_pool_coarsen_static(batch.x, batch, S.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="asap_static: edge_weight requires grad"):
        tfg.nn.asap_static(tracked.x, tracked, *ws, k=3)


# ---- 9. the example ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [("--static", "--capture"), ("--static",), ()], ids=["capture", "static", "default"])
def test_demo_runs_and_trains(flags):
    """In a fresh child process: a few steps, finite losses that move from epoch to epoch.  "default": main() of the example was
    edited for the two flags, and without them the program must be what it was."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "demo_asap.py")] + list(flags) +
                       ["--graphs", "80", "--epochs", "3", "--batch-size", "8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("epoch")]
    print(r.stdout[-800:])
    losses = [float(line.split("loss")[1].split()[0]) for line in lines]
    assert len(losses) == 3 and np.isfinite(losses).all() and len(set(losses)) == 3, r.stdout[-1500:]
    assert ("replayed" in r.stdout) == ("--capture" in flags)
