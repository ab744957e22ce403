# coding=utf-8
"""include/tfgx_asap_static.h without a GPU: names and macros against _lib, every refusal (on the host, the argument named), the
zero-size calls, the numpy mirror of the pooled layout (tests/asap_static_mirror.py) against a stable sort and against the pooled
edge set of the float64 ASAP mirror (tests/asap_mirror.py) for the same graphs, and StaticBatchGraph.asap_pooled_capacities
against a brute force over every batch of a small store."""
import ctypes
import itertools

import numpy as np
import pytest

from abi_header import declarations, macro, refused as _refused
from asap_mirror import asap_mirror, make_weights
from asap_static_mirror import mirror_asap_capacities, mirror_asap_layout, mirror_assignment, mirror_clusters
from densepool_static_mirror import mirror_pooled_weight
from test_drop_edge_abi import mirror_plan

HEADER = "tfgx_asap_static.h"


def test_asap_static_names_and_constants():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.ASAPSTATIC_SIGNATURES) == [
        "tfgx_asapstatic_assign_f32", "tfgx_asapstatic_attend_backward_f32", "tfgx_asapstatic_attend_f32", "tfgx_asapstatic_edges",
        "tfgx_asapstatic_edges_workspace_bytes", "tfgx_asapstatic_version"]
    for abi in L.ABIS:
        assert abi.signatures is L.ASAPSTATIC_SIGNATURES or not any("asapstatic" in n for n in abi.signatures), abi.header
    assert macro(HEADER, "TFGX_ASAPSTATIC_ABI_VERSION") == L.ASAPSTATIC_ABI_VERSION == 1
    assert L.load_library().tfgx_asapstatic_version() == 1
    assert macro(HEADER, "TFGX_ASAPSTATIC_MAX_K") == L.ASAPSTATIC_MAX_K == L.SEGGRAM_MAX_K == 64
    assert macro("tfgx_seggram.h", "TFGX_SEGGRAM_MAX_K") == L.ASAPSTATIC_MAX_K
    assert macro(HEADER, "TFGX_ASAPSTATIC_MAX_FEATURES") == L.ASAPSTATIC_MAX_FEATURES == L.ASAP_MAX_FEATURES
    assert macro("tfgx_asap.h", "TFGX_ASAP_MAX_FEATURES") == L.ASAPSTATIC_MAX_FEATURES
    assert macro(HEADER, "TFGX_ASAPSTATIC_MAX_SLOTS") == L.ASAPSTATIC_MAX_SLOTS == L.STATIC_POOL_MAX_SLOTS
    # the headers this one must not touch are where they were
    assert macro("tfgx.h", "TFGX_ABI_VERSION") == L.ABI_VERSION == 114 and macro("tfgx_asap.h", "TFGX_ASAP_ABI_VERSION") == 1
    assert L.AsapStaticEdgesArgs is L.STRUCTS["tfgx_asapstatic_edges_args"]


# ---- (a) the attention ------------------------------------------------------------------------------------------------------------
ATT_OK = dict(row_ptr=8, col=8, N=4, E=6, x=8, ldx=16, F=16, sq=8, sh=8, bias=8, drop_rate=0.0, seed=0, seed_dev=None, skip=1, c=8,
              ldc=16, p=8, p_self=8, p_drop=None, p_self_drop=None, flag=None, stream=None)


@pytest.mark.parametrize("change, word", [
    (dict(N=-1), "negative size (N"), (dict(E=-1), "negative size (E"), (dict(F=-1), "negative size (F"),
    (dict(N=1 << 31), "N = 2147483648 does not fit int32"), (dict(N=1 << 30, E=1 << 30), "N + E = 2147483648 does not fit int32"),
    (dict(F=257, ldx=257, ldc=257), "F exceeds TFGX_ASAPSTATIC_MAX_FEATURES"), (dict(ldx=15), "ldx is smaller than F"),
    (dict(ldc=15), "ldc is smaller than F"), (dict(drop_rate=1.0), "drop_rate"), (dict(drop_rate=-0.1), "drop_rate"),
    (dict(drop_rate=float("nan")), "drop_rate"),
    (dict(row_ptr=None), "row_ptr is null"), (dict(col=None), "col is null"), (dict(x=None), "x is null"),
    (dict(sq=None), "sq is null"), (dict(sh=None), "sh is null"), (dict(bias=None), "bias is null"), (dict(c=None), "c is null"),
    (dict(p=None), "p is null"), (dict(p_self=None), "p_self is null"), (dict(drop_rate=0.5), "p_drop is null"),
    (dict(drop_rate=0.5, p_drop=8), "p_self_drop is null"),
])
def test_attend_argument_checks_name_the_member(change, word):
    _refused("tfgx_asapstatic_attend_f32", ATT_OK, change, word)


BWD_OK = dict(row_ptr=8, col=8, N=4, E=6, sq=8, sh=8, bias=8, p=8, p_self=8, p_drop=None, p_self_drop=None, dp=8, dp_self=8, skip=1,
              ds=8, ds_self=8, dsq=8, stream=None)


@pytest.mark.parametrize("change, word", [
    (dict(N=-1), "negative size (N"), (dict(N=1 << 31), "does not fit int32"), (dict(row_ptr=None), "row_ptr is null"),
    (dict(col=None), "col is null"), (dict(sq=None), "sq is null"), (dict(sh=None), "sh is null"), (dict(bias=None), "bias is null"),
    (dict(p=None), "p is null"), (dict(p_self=None), "p_self is null"), (dict(p_drop=8), "both p_drop and p_self_drop"),
    (dict(p_self_drop=8), "both p_drop and p_self_drop"), (dict(E=0, p_drop=8), "both p_drop and p_self_drop"),
    (dict(dp=None), "dp is null"), (dict(dp_self=None), "dp_self is null"), (dict(ds=None), "ds is null"),
    (dict(ds_self=None), "ds_self is null"), (dict(dsq=None), "dsq is null"),
])
def test_attend_backward_argument_checks_name_the_member(change, word):
    _refused("tfgx_asapstatic_attend_backward_f32", BWD_OK, change, word)


# ---- (b) the assignment -----------------------------------------------------------------------------------------------------------
ASSIGN_OK = dict(row_ptr=8, col=8, N=10, E=6, p=8, p_self=8, skip=1, node_index=8, pooled_ngi=8, prp=8, B=2, m_rows=4, K=3, S=8, lds=3,
                 stream=None)


@pytest.mark.parametrize("change, word", [
    (dict(N=-1), "negative size (N"), (dict(E=-1), "negative size (E"), (dict(B=-1), "negative size (B"),
    (dict(m_rows=-1), "negative size (m_rows"), (dict(K=-1), "negative size (K"), (dict(lds=-1), "negative size (lds"),
    (dict(N=1 << 31), "N = 2147483648 does not fit int32"), (dict(K=65, lds=65), "K = 65 is more than 64"),
    (dict(lds=2), "lds is smaller than K"), (dict(S=None), "S is null"), (dict(row_ptr=None), "row_ptr is null"),
    (dict(col=None), "col is null"), (dict(p=None), "p is null"), (dict(p_self=None), "p_self is null"),
    (dict(node_index=None), "node_index is null"), (dict(pooled_ngi=None), "pooled_node_graph_index is null"),
    (dict(prp=None), "pooled_row_ptr is null"),
])
def test_assign_argument_checks_name_the_member(change, word):
    """Every refusal comes before S is zeroed: the pointers here are not memory."""
    _refused("tfgx_asapstatic_assign_f32", ASSIGN_OK, change, word)


# ---- (c) the pooled edges ---------------------------------------------------------------------------------------------------------
# B = 8 slots of at most K = 5 clusters, 30 rows + 5 sinks of degree 32 for 150 edges
FAKE = dict(P=1 << 30, ldp=5, pooled_row_ptr=2 << 30, B=8, K=5, n_cap_out=35, e_cap=150, sinks=5, sink_degree=32, out_row=8 << 30,
            out_col=9 << 30, out_edge_src=10 << 30, out_edge_graph_index=11 << 30, counts=12 << 30, workspace=13 << 30,
            workspace_bytes=1 << 20)
FAKE_PLAN = dict(out_row_ptr=14 << 30, out_col=15 << 30, out_perm=16 << 30)


def _call(lib, plan=FAKE_PLAN, plan_t=FAKE_PLAN, **kw):
    from tf_geometric_amd import _lib as L
    a = L.AsapStaticEdgesArgs(**dict(FAKE, **kw))
    keep = []
    for name, p in (("plan", plan), ("plan_t", plan_t)):
        if p is not None:
            keep.append(L.CollatePlan(**p))
            setattr(a, name, ctypes.pointer(keep[-1]))
    return lib.tfgx_asapstatic_edges(ctypes.byref(a), None)


def test_edges_argument_validation_without_gpu():
    """Every refusal returns TFGX_ERR_INVALID_ARG (1) on the host, before any device work (the pointers are not memory), with
    the entry point and the argument named."""
    from tf_geometric_amd import _lib as L
    lib = L.load_library()

    def refused(rc, word, code=1):
        assert rc == code, (rc, word)
        msg = lib.tfgx_last_error()
        assert word in msg and b"tfgx_asapstatic_edges:" in msg, (word, msg)

    refused(lib.tfgx_asapstatic_edges(None, None), b"args is null")
    for member in ("B", "K", "ldp", "n_cap_out", "e_cap", "sinks", "sink_degree"):
        refused(_call(lib, **{member: -1}), b"negative size (" + member.encode())
        refused(_call(lib, **{member: 1 << 31}), member.encode() + b" = 2147483648 does not fit int32")
    refused(_call(lib, B=L.ASAPSTATIC_MAX_SLOTS + 1), b"B = 1048577 is more than the 1048576 slots")
    refused(_call(lib, K=65, ldp=65), b"K = 65 is more than 64")
    refused(_call(lib, ldp=4), b"ldp is smaller than K")
    refused(_call(lib, sink_degree=0), b"sink_degree = 0 must be at least 1")
    refused(_call(lib, sinks=36), b"sinks = 36 is more than n_cap_out = 35 rows")
    refused(_call(lib, sinks=4), b"sinks = 4 of sink_degree = 32 cannot hold a tail of e_cap = 150")
    refused(_call(lib, e_cap=149), b"e_cap = 149 is smaller than K * (n_cap_out - sinks) = 150")
    refused(_call(lib, B=1 << 20, K=64, ldp=64), b"B * K * K = 4294967296 does not fit int32")
    for member in ("counts", "pooled_row_ptr", "workspace", "P", "out_row", "out_col", "out_edge_src", "out_edge_graph_index"):
        refused(_call(lib, **{member: None}), member.encode() + b" is null")
    refused(_call(lib, plan=None), b"plan is null")
    refused(_call(lib, plan_t=None), b"plan_t is null")
    for member in FAKE_PLAN:
        p = dict(FAKE_PLAN, **{member: None})
        refused(_call(lib, plan=p), b"plan->" + member.encode() + b" is null")
        refused(_call(lib, plan_t=p), b"plan_t->" + member.encode() + b" is null")
    need = lib.tfgx_asapstatic_edges_workspace_bytes(8)
    assert need > 0 and lib.tfgx_asapstatic_edges_workspace_bytes(-1) == 0
    assert lib.tfgx_asapstatic_edges_workspace_bytes(L.ASAPSTATIC_MAX_SLOTS + 1) == 0
    refused(_call(lib, workspace_bytes=need - 1), b"workspace_bytes", code=3)          # TFGX_ERR_WORKSPACE


def test_zero_size_calls_succeed_without_gpu():
    """Where nothing exists to be written nothing is launched."""
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    nothing = {k: None for k, v in FAKE.items() if v >= 1 << 30}
    for K in (0, 1, 5, 64):
        rc = _call(lib, plan=None, plan_t=None, **dict(nothing, B=0, K=K, ldp=K, n_cap_out=0, e_cap=0, sinks=0, workspace_bytes=0))
        assert rc == 0, lib.tfgx_last_error().decode()
    none = {k: None for k, v in ATT_OK.items() if v == 8}
    assert lib.tfgx_asapstatic_attend_f32(*dict(ATT_OK, **dict(none, N=0, E=0)).values()) == 0
    none = {k: None for k, v in BWD_OK.items() if v == 8}
    assert lib.tfgx_asapstatic_attend_backward_f32(*dict(BWD_OK, **dict(none, N=0, E=0)).values()) == 0
    none = {k: None for k, v in ASSIGN_OK.items() if v == 8}
    assert lib.tfgx_asapstatic_assign_f32(*dict(ASSIGN_OK, **dict(none, N=0, E=0)).values()) == 0
    assert lib.tfgx_asapstatic_assign_f32(*dict(ASSIGN_OK, **dict(none, K=0, lds=0)).values()) == 0


# ---- the mirror's closed-form plans are stable sorts -----------------------------------------------------------------------------
def _random_blocks(rng, B, K, density):
    P = rng.integers(1, 4, (B * K, K)).astype(np.float32) * (rng.random((B * K, K)) < density)
    if P.size >= 2:
        P.reshape(-1)[1], P.reshape(-1)[-2] = -0.0, np.nan
    return P


@pytest.mark.parametrize("sink_degree", [1, 32])
@pytest.mark.parametrize("K", [0, 1, 3, 20, 64])
def test_mirror_plans_are_the_stable_sorts_of_its_list_and_of_the_flip(K, sink_degree):
    rng = np.random.Generator(np.random.PCG64(K * 4 + sink_degree))
    for B in (5, 1, 0):
        for density in (0.0, 0.4, 1.0):
            P = _random_blocks(rng, B, K, density)
            m = rng.integers(0, K + 1, B)
            if B:
                m[rng.integers(0, B)] = K                        # one slot is full, and some are empty
            prp = np.concatenate([[0], np.cumsum(m)]).astype(np.int32)
            m_max = int(prp[-1]) + 3
            e_cap = K * m_max
            sinks = max(1, -(-e_cap // sink_degree))
            n_cap = m_max + sinks
            lay = mirror_asap_layout(P, np.concatenate([prp, [n_cap]]), [B, prp[-1], 0, 2], K, n_cap, e_cap, sinks, sink_degree)
            ei, e = lay["edge_index"], lay["e_live"]
            for got, ref in ((lay["plan"], mirror_plan(ei, n_cap)), (lay["plan_t"], mirror_plan(ei[::-1], n_cap))):
                for a, b in zip(got, ref):
                    assert np.array_equal(a, b)
            assert (np.diff(ei[0]) >= 0).all()                   # sorted by row: the plan by row is the list
            assert list(lay["counts"]) == [B, prp[-1], e, 2] and e >= prp[-1]
            src = lay["edge_src"][:e]
            loops = ei[0, :e] == ei[1, :e]
            assert np.array_equal(src < 0, loops) and loops.sum() == prp[-1]          # one unit self-loop per live row, no other
            if K:
                kept = P.reshape(-1)[src[~loops]]
                assert ((kept != 0) | np.isnan(kept)).all()
                assert np.array_equal(lay["edge_graph_index"][:e][~loops], src[~loops] // (K * K))
            # the self-loop is the LAST entry of its row, the others are in column order
            for r in range(int(prp[-1])):
                seg = ei[1, lay["plan"][0][r]:lay["plan"][0][r + 1]]
                assert seg[-1] == r and (np.diff(seg[:-1]) > 0).all() and r not in seg[:-1]
            assert (ei[:, e:] >= m_max).all() and (ei[0, e:] == ei[1, e:]).all() and (lay["edge_graph_index"][e:] == B).all()
            assert np.bincount(ei[0, e:], minlength=n_cap).max(initial=0) <= sink_degree


# ---- the mirror is the ASAP mirror's pooled graph --------------------------------------------------------------------------------
SIZES = [0, 1, 4, 7, 12, 3]


def _graphs(rng):
    """A batch as numpy: x, edge_index (with duplicates and self-loops), positive weights, graph ids."""
    xs, eis, ws, gid, off = [], [], [], [], 0
    for g, n in enumerate(SIZES):
        xs.append(rng.standard_normal((n, 5)).astype(np.float32))
        e = 0 if n < 2 else 3 * n
        a, b = rng.integers(0, max(n, 1), e), rng.integers(0, max(n, 1), e)
        eis.append(np.stack([a, b]) + off)
        ws.append(rng.uniform(0.5, 1.5, e).astype(np.float32))
        gid.append(np.full(n, g))
        off += n
    return np.concatenate(xs), np.concatenate(eis, axis=1).astype(np.int32), np.concatenate(ws), np.concatenate(gid)


@pytest.mark.parametrize("k,ratio", [(1, None), (3, None), (64, None), (None, 0.5)])
def test_mirror_live_part_is_the_asap_mirror_pooled_graph(k, ratio):
    rng = np.random.Generator(np.random.PCG64(11))
    x, ei, w, gid = _graphs(rng)
    ref = asap_mirror(x, ei, w, gid, make_weights(rng, 5, 4), k=k, ratio=ratio)
    B = len(SIZES) + 1                                           # a dead slot last
    m = [mirror_clusters(n, k, ratio) for n in SIZES] + [0]
    K = max(m)
    prp = np.concatenate([[0], np.cumsum(m)]).astype(np.int32)
    assert prp[-1] == ref["idx"].shape[0] and np.array_equal(np.repeat(np.arange(B), m), ref["node_graph_index"])
    Pd = ref["P"].numpy()
    P = np.full((B * K, K), 7.0, np.float32)                      # what lies beyond m_g must not matter
    for g in range(B):
        P[g * K:g * K + m[g], :m[g]] = Pd[prp[g]:prp[g + 1], prp[g]:prp[g + 1]]
    assert np.count_nonzero(Pd) == sum(np.count_nonzero(Pd[prp[g]:prp[g + 1], prp[g]:prp[g + 1]]) for g in range(B))
    m_max = int(prp[-1]) + 2
    e_cap = K * m_max
    sinks = max(1, -(-e_cap // 32))
    lay = mirror_asap_layout(P, np.concatenate([prp, [m_max + sinks]]), [B - 1, prp[-1], 0, 0], K, m_max + sinks, e_cap, sinks, 32)
    e = lay["e_live"]
    # nn.asap's list is [off-diagonal entries row-major; the diagonal]: its CSR plan walks a row in the stable sort by row
    order = np.argsort(ref["edge_index"][0], kind="stable")
    assert e == order.shape[0] and np.array_equal(lay["edge_index"][:, :e], ref["edge_index"][:, order])
    got = mirror_pooled_weight(P, lay["edge_src"])[:e]
    want = ref["edge_weight"].numpy()[order]
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()


def test_mirror_assignment_is_the_asap_mirror_assignment():
    """S of the header (per column the edges of the centre's row in CSR order, self-loops absent, p_self last) against the dense
    assignment the float64 mirror builds: S^T A1 S of it is the mirror's P."""
    rng = np.random.Generator(np.random.PCG64(12))
    x, ei, w, gid = _graphs(rng)
    ref = asap_mirror(x, ei, w, gid, make_weights(rng, 5, 4), k=3)
    n, B = x.shape[0], len(SIZES)
    row_ptr, col, perm = mirror_plan(ei, n)                      # self-loops stay in the list: they are absent by the rule
    E0 = int((ei[0] != ei[1]).sum())
    p64 = ref["p"].numpy()
    p_edges = np.zeros(ei.shape[1])
    p_edges[np.flatnonzero(ei[0] != ei[1])] = p64[:E0]           # the mirror's p is in the order of the self-loop-free list
    p_csr, p_self = p_edges[perm].astype(np.float32), p64[E0:].astype(np.float32)
    m = [mirror_clusters(s, 3, None) for s in SIZES]
    prp = np.concatenate([[0], np.cumsum(m)]).astype(np.int32)
    S = mirror_assignment(row_ptr, col, p_csr, p_self, ref["idx"], np.repeat(np.arange(B), m), prp, B, 3)
    A1 = np.zeros((n, n))
    keep = ei[0] != ei[1]
    np.add.at(A1, (ei[0][keep], ei[1][keep]), w[keep].astype(np.float64))
    A1 += np.eye(n)
    Pd = ref["P"].numpy()
    for g in range(B):
        nodes = np.flatnonzero(gid == g)
        Sg = S[nodes][:, :m[g]].astype(np.float64)
        block = Sg.T @ A1[np.ix_(nodes, nodes)] @ Sg
        want = Pd[prp[g]:prp[g + 1], prp[g]:prp[g + 1]]
        assert np.abs(block - want).max(initial=0.0) <= 1e-6 * max(np.abs(want).max(initial=0.0), 1.0)


# ---- the capacities ---------------------------------------------------------------------------------------------------------
def _static_batch(sizes, B, sink_degree, node_bound=None):
    """A StaticBatchGraph of B slots over a store of graphs with `sizes` nodes (host arrays only: no device is touched)."""
    import torch
    import tf_geometric_amd as tfg
    from tf_geometric_amd.data import graph as G
    store = tfg.data.GraphStore([tfg.Graph(np.zeros((n, 1), np.float32), np.zeros((2, 0), np.int32)) for n in sizes])
    cap = store.static_capacities(B, sink_degree=sink_degree)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)      # noqa: E731
    batch = G.StaticBatchGraph(torch.zeros((cap.n_cap, 1)), torch.zeros((2, cap.e_cap), dtype=torch.int32), i32(cap.n_cap),
                               i32(cap.e_cap), None, None, i32(B), torch.ones(B, dtype=torch.bool), i32(4), cap, len(sizes))
    batch._store, batch._node_bound = store, node_bound
    return batch


STORE_SIZES = [0, 1, 2, 3, 5, 10, 10, 33]


@pytest.mark.parametrize("k,ratio", [(0, None), (1, None), (3, None), (64, None), (None, 0.5), (None, 0.1), (None, 0.3),
                                     (None, 1.0), (None, 0.0), (None, 0.7)])
@pytest.mark.parametrize("d", [1, 32])
def test_asap_pooled_capacities_against_brute_force(k, ratio, d):
    """Every batch of distinct graphs of the store (dead slots included: fewer graphs than slots) keeps at most K_blk clusters
    of a graph, max_nodes rows and — sum m_g^2 <= K_blk sum m_g — max_edges edges; K_blk is reached.  ratio 0.1 on 10 nodes is
    where float32(10) * float32(0.1) rounds to 1.0f while the exact product of the two is above 1: the kernel keeps 1."""
    assert mirror_clusters(10, None, 0.1) == 1
    for B in (0, 1, 2, 3):
        batch = _static_batch(STORE_SIZES, B, d)
        cap = batch.asap_pooled_capacities(k=k, ratio=ratio)
        K = batch.asap_clusters_per_graph(k=k, ratio=ratio)
        assert (K, cap.max_nodes, cap.max_edges, cap.sinks, cap.n_cap, cap.e_cap) == mirror_asap_capacities(
            B, batch.capacities.max_nodes, max(STORE_SIZES), d, k, ratio)
        assert cap.batch_size == B and cap.sink_degree == d and cap.n_cap == cap.max_nodes + cap.sinks and cap.e_cap == cap.max_edges
        assert cap.sinks >= 1 and cap.sinks * d >= cap.e_cap and (cap.sinks - 1) * d < max(cap.e_cap, 1)
        assert cap.max_nodes == batch.pooled_capacities(k=k, ratio=ratio).max_nodes
        most = 0
        for live in range(B + 1):
            for ids in itertools.combinations(range(len(STORE_SIZES)), live):
                m = [mirror_clusters(STORE_SIZES[i], k, ratio) for i in ids]
                most = max([most] + m)
                assert sum(m) <= cap.max_nodes and sum(v * v for v in m) <= cap.max_edges and max(m, default=0) <= K
        assert most == (K if B else 0)
    # after a pooling level the bound is the previous level's, not the store's
    assert _static_batch(STORE_SIZES, 3, d, node_bound=7).asap_clusters_per_graph(k=k, ratio=ratio) == mirror_clusters(7, k, ratio)


def test_asap_pooled_capacities_refusals():
    batch = _static_batch(STORE_SIZES, 4, 32)
    for kw in (dict(), dict(k=1, ratio=0.5)):
        with pytest.raises(ValueError, match="either k or ratio"):
            batch.asap_pooled_capacities(**kw)
    for bad in (-1, 2.0, True):
        with pytest.raises(ValueError, match="k must be"):
            batch.asap_pooled_capacities(k=bad)
    for bad in (-0.5, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="ratio must be"):
            batch.asap_pooled_capacities(ratio=bad)
    big = _static_batch([40000] * 2, 2, 1, node_bound=40000)
    with pytest.raises(ValueError, match="int32"):
        big.asap_pooled_capacities(ratio=1.0)                    # 80000 rows of 40000 edges each
