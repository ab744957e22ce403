# coding=utf-8
"""The device-side plan builders (tfgx_plan_row_order, tfgx_plan_hub_lists_count / _emit, tfgx_plan_hub_order_slot,
tfgx_plan_source_blocks) held BIT-IDENTICAL to the torch statements the plan used to run — kept verbatim below as the
reference — on uniform, dense, R-MAT and rectangular graphs, graphs with empty rows, empty plans, a 10^5-edge row and the
Reddit shape.  Index work: no tolerance."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KBS = (1, 2, 3, 5, 11, 16, 64)


# ---- the torch bodies of CsrPlan.row_order / source_blocks / hub_order_slot before the device builders (verbatim) ----------
def _ref_row_order(plan):
    order = False
    if plan.n_dst > 0 and plan.num_edges > 0:
        deg = plan.in_degree()
        if int(deg.max().item()) > 8 * max(plan.num_edges / float(plan.n_dst), 1.0):
            order = torch.argsort(deg, descending=True, stable=True).to(torch.int32).contiguous()
    return None if order is False else order


def _ref_source_blocks(plan, KB):
    dev = plan.col.device
    blk = max(-(-plan.n_src // KB), 1)
    rows = torch.repeat_interleave(torch.arange(plan.n_dst, device=dev, dtype=torch.int64), plan.in_degree().long())
    key = rows * KB + torch.div(plan.col.long(), blk, rounding_mode="floor")
    del rows
    order = torch.argsort(key, stable=True)
    rpk = torch.zeros(plan.n_dst * KB + 1, dtype=torch.int32, device=dev)
    rpk[1:] = torch.cumsum(torch.bincount(key, minlength=plan.n_dst * KB), 0).to(torch.int32)
    del key
    return rpk, plan.col[order].contiguous()


def _ref_hub_order_slot(hub, order):
    n_hub = int(hub[0].shape[0])
    return torch.searchsorted(hub[0], order[:n_hub].contiguous()).to(torch.int32).contiguous()


def _ref_strided_hub_lists(row_begin, row_end, rp_stride, n_dst, thr, chunk):
    """What dist/sharded.py:HipBackend.hub_lists computes: the strided spans gathered with an index tensor first."""
    from tf_geometric_amd.plan import build_hub_lists
    idx = torch.arange(n_dst, device=row_begin.device) * rp_stride
    return build_hub_lists(row_begin[idx], row_end[idx], thr, chunk)


def _same(got, want, what):
    if want is None:
        assert got is None, what
        return
    assert got is not None, what
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.int32 and g.shape == w.shape, (what, i, g.dtype, g.shape, w.shape)
        assert torch.equal(g, w.to(torch.int32)), (what, i)


# ---- graphs -------------------------------------------------------------------------------------------------------------
def _uniform(n_dst, n_src, e, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    row = torch.randint(0, max(n_dst, 1), (e,), device="cuda", generator=g, dtype=torch.int64)
    col = torch.randint(0, max(n_src, 1), (e,), device="cuda", generator=g, dtype=torch.int64)
    return torch.stack([row, col]).to(torch.int32)


def _dense(n, deg, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    row = torch.arange(n, device="cuda").repeat_interleave(deg)
    col = torch.randint(0, n, (n * deg,), device="cuda", generator=g)
    return torch.stack([row, col]).to(torch.int32)


def _graph(kind):
    from tf_geometric_amd import synthetic
    if kind == "uniform":
        return _uniform(3000, 3000, 40000, 1), 3000, 3000
    if kind == "dense":
        return _dense(2000, 97, 2), 2000, 2000
    if kind == "rmat":
        n = 1 << 14
        return synthetic.rmat_edges(n, 300000, 3, torch.device("cuda")), n, n
    if kind == "empty_rows":          # only even destinations have edges, the last 100 rows none
        ei = _uniform(2500, 4000, 60000, 4)
        ei[0] = (ei[0] // 2) * 2
        return ei, 2600, 4000
    if kind == "n_src_below_kb":      # n_src < KB for most KB
        return _uniform(500, 7, 20000, 5), 500, 7
    if kind == "n_src_odd":           # n_src not a multiple of KB
        return _uniform(777, 1001, 50000, 6), 777, 1001
    if kind == "no_edges":
        return torch.zeros((2, 0), dtype=torch.int32, device="cuda"), 300, 300
    if kind == "no_rows":
        return torch.zeros((2, 0), dtype=torch.int32, device="cuda"), 0, 50
    raise KeyError(kind)


KINDS = ["uniform", "dense", "rmat", "empty_rows", "n_src_below_kb", "n_src_odd", "no_edges", "no_rows"]


@pytest.mark.parametrize("kind", KINDS)
def test_source_blocks_bit_identical(tfg, kind):
    from tf_geometric_amd.plan import CsrPlan
    ei, n_dst, n_src = _graph(kind)
    plan = CsrPlan.build(ei, n_dst, n_src)
    for KB in KBS:
        rpk, col_k = plan.source_blocks(KB)
        want = _ref_source_blocks(plan, KB)
        _same((rpk, col_k), want, "{} KB={}".format(kind, KB))
        assert int(rpk[-1].item()) == plan.num_edges
        assert plan.source_blocks(KB)[0] is rpk          # memoised per (plan, KB)


def test_source_blocks_hub_row_of_1e5_edges(tfg):
    """One destination with 150 000 in-edges (one wave walks it) among ordinary rows."""
    from tf_geometric_amd.plan import CsrPlan
    n = 20000
    ei = _uniform(n, n, 200000, 7)
    g = torch.Generator(device="cuda")
    g.manual_seed(8)
    hub = torch.stack([torch.full((150000,), 4321, device="cuda", dtype=torch.int64),
                       torch.randint(0, n, (150000,), device="cuda", generator=g)]).to(torch.int32)
    ei = torch.cat([ei, hub], 1)
    plan = CsrPlan.build(ei, n, n)
    assert int(plan.in_degree().max().item()) > 100000
    for KB in (2, 3, 16, 64):
        _same(plan.source_blocks(KB), _ref_source_blocks(plan, KB), "hub row KB={}".format(KB))


@pytest.mark.parametrize("kind", KINDS + ["ties"])
def test_row_order_bit_identical(tfg, kind):
    from tf_geometric_amd.plan import CsrPlan
    if kind == "ties":       # degrees 3 or 4 everywhere (long runs of equal keys) and one long row: skewed
        n = 5000
        row = torch.arange(n, device="cuda").repeat_interleave(3 + (torch.arange(n, device="cuda") % 7 == 0).long())
        row = torch.cat([row, torch.full((1000,), 17, device="cuda", dtype=torch.int64)])
        ei = torch.stack([row, row * 31 % n]).to(torch.int32)
        n_dst = n_src = n
    else:
        ei, n_dst, n_src = _graph(kind)
    plan = CsrPlan.build(ei, n_dst, n_src)
    want = _ref_row_order(plan)
    got = plan.row_order()
    if kind in ("uniform", "dense", "no_edges", "no_rows", "n_src_odd"):
        assert want is None        # near-regular / empty: "no order"
    if kind in ("rmat", "ties"):
        assert want is not None
    if want is None:
        assert got is None
    else:
        assert got.dtype == torch.int32 and torch.equal(got, want), kind


@pytest.mark.parametrize("kind", ["rmat", "uniform", "empty_rows", "no_edges"])
def test_hub_lists_bit_identical(tfg, kind):
    from tf_geometric_amd import plan as P
    ei, n_dst, n_src = _graph(kind)
    plan = P.CsrPlan.build(ei, n_dst, n_src)
    thr, chunk = P.hub_policy(plan.num_edges, plan.n_dst)
    rb, re_ = plan.row_ptr[:-1], plan.row_ptr[1:]
    _same(plan.hub_info(), P.build_hub_lists(rb, re_, thr, chunk), kind + " plan policy")
    if kind == "rmat":
        assert plan.hub_info() is not None
    for t, c in ((64, 48), (0, 1), (5, 3)):
        _same(P.build_hub_lists_device(plan.row_ptr, plan.row_ptr[1:], 1, plan.n_dst, t, c),
              P.build_hub_lists(rb, re_, t, c), "{} forced {}/{}".format(kind, t, c))
    # strided spans (rp_stride = 2): the source-block partition's per-block spans, as the sharded path passes them
    if plan.n_dst > 0:
        rpk, _ = plan.source_blocks(2)
        for k in range(2):
            for t, c in ((thr, chunk), (64, 48)):
                _same(P.build_hub_lists_device(rpk[k:], rpk[k + 1:], 2, plan.n_dst, t, c),
                      _ref_strided_hub_lists(rpk[k:], rpk[k + 1:], 2, plan.n_dst, t, c), "{} stride 2 block {}".format(kind, k))


def test_sharded_backend_hub_lists(tfg):
    """The strided builder reproduces the sharded backend's per-class hub lists (spans rpk[k::K]) bit for bit, reading the
    spans in place instead of gathering them."""
    from tf_geometric_amd import plan as P
    from tf_geometric_amd.dist.sharded import HipBackend
    ei, n, _ = _graph("rmat")
    plan = P.CsrPlan.build(ei, n, n)
    rpk, _ = plan.source_blocks(3)
    be = HipBackend()
    thr, chunk = P.hub_policy(plan.num_edges, n)
    seen = 0
    for k in range(3):
        want = be.hub_lists(rpk[k:], rpk[k + 1:], 3, n, plan.num_edges)
        got = P.build_hub_lists_device(rpk[k:], rpk[k + 1:], 3, n, thr, chunk)
        if want is None:
            assert got is None
        else:
            assert want[0] == thr
            _same(got, want[1:], "sharded block {}".format(k))
            seen += 1
    assert seen > 0


def test_hub_order_slot_bit_identical(tfg):
    from tf_geometric_amd import plan as P
    ei, n, _ = _graph("rmat")
    plan = P.CsrPlan.build(ei, n, n)
    hub, order = plan.hub_info(), plan.row_order()
    assert hub is not None and order is not None
    slot = plan.hub_order_slot()
    want = _ref_hub_order_slot(hub, order)
    assert slot.dtype == torch.int32 and torch.equal(slot, want)
    assert torch.equal(hub[0][slot.long()], order[:int(hub[0].shape[0])])     # the walk order's first rows ARE the hubs
    # forced lists that do not start the walk order (not all long rows are hubs): still the searchsorted result
    lists = P.build_hub_lists(plan.row_ptr[:-1], plan.row_ptr[1:], 2048, 1024)
    if lists is not None:
        out = torch.empty(int(lists[0].shape[0]), dtype=torch.int32, device="cuda")
        tfg._lib.check(tfg._lib.load_library().tfgx_plan_hub_order_slot(
            tfg._lib.ptr(lists[0]), int(lists[0].shape[0]), tfg._lib.ptr(order), tfg._lib.ptr(out), tfg._lib.stream_ptr()))
        assert torch.equal(out, _ref_hub_order_slot(lists, order))
    # a plan without hub rows or walk order has no slot
    plan_u = P.CsrPlan.build(*_graph("uniform")[:2])
    assert plan_u.hub_order_slot() is None


def _timed(fn, reps=3):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        del out
    return best


def test_reddit_shape_source_blocks(tfg):
    """233 k destinations x 489 in-edges, KB from the policy: bit-identical to the torch build.  Times are printed."""
    from tf_geometric_amd.plan import CsrPlan
    from tf_geometric_amd.nn.conv import gat as G
    from tf_geometric_amd import synthetic
    n, e, _ = synthetic.WORKLOADS["reddit"]
    ei = _dense(n, e // n, 11)
    plan = CsrPlan.build(ei, n, n)
    del ei
    assert G.SOURCE_BLOCKS is None
    KB = G.source_block_count(plan, 8, 64)
    assert KB >= 2
    got = plan.source_blocks(KB)
    _same(got, _ref_source_blocks(plan, KB), "reddit KB={}".format(KB))
    lib = tfg._lib.load_library()
    rpk, col_k = torch.empty_like(got[0]), torch.empty_like(got[1])

    def device_build():
        tfg._lib.check(lib.tfgx_plan_source_blocks(tfg._lib.ptr(plan.row_ptr), tfg._lib.ptr(plan.col), plan.n_dst, plan.n_src,
                                                   plan.num_edges, KB, tfg._lib.ptr(rpk), tfg._lib.ptr(col_k),
                                                   tfg._lib.stream_ptr()))
    ms_dev = _timed(device_build)
    ms_torch = _timed(lambda: _ref_source_blocks(plan, KB))
    assert torch.equal(rpk, got[0]) and torch.equal(col_k, got[1])
    print("\nreddit-shape source blocks (n={}, E={}, KB={}): device {:.3f} ms, torch {:.3f} ms".format(
        n, plan.num_edges, KB, ms_dev, ms_torch))
