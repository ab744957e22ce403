# coding=utf-8
"""plan.segment_reduce / plan.aggregate_gemm against a hand-filled call of the same C entry.

Every case calls the Python entry and, separately, the library entry with a tfgx_reduce_args this module fills itself (an
independent C-ABI host, as test_gpu_fuzz_forward's census and test_gpu_fused_h16's launch()).  Which optional members a
launch carries is stated here from the entry's contract, not asked of plan.py:
  * hub lists (with a scratch of their own): launches over the plan's own rows — no explicit row_begin / row_end / col and
    n_dst == plan.n_dst — and, on the float32 entry, no `track`;
  * the walk order: segment_reduce on its own rows at F <= plan.ROW_ORDER_MAX_F; aggregate_gemm whenever the plan has one,
    together with hub_order_slot;
  * wide_blocks: plan.wide_blocks_hint for a float32 table, plan.h16_wide_blocks_hint for a HalfRows, the caller's
    wide_blocks= over either.
Required: torch.equal on every output (out, agg_out, track; a 16-bit output bit for bit), equal describe strings, and
every launch counter moving by exactly its stated amount.  The shapes are the smallest at which the fill can go wrong: 70
destinations (one empty, one with 300 in-edges: hub lists, a walk order and a hub_order_slot), the same graph without the
long row, and 8 destinations x 300 edges at F = 256, where the column-block shapes are reachable."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_fuzz_backward import _degrees, _graph, _hubs, _rng, _skewed
from test_gpu_h16 import _bits16, _fill16, _nan32

pytestmark = pytest.mark.gpu
N, EMPTY_ROW, HUB_ROW = 70, 5, 11
BF16, FP16 = torch.bfloat16, torch.float16


# ------------------------------------------------------------------------------------------------------------------ graphs
def _edges(name):
    """'plain': _graph's duplicate edges and self-loops on 70 x 70, destination 5 left empty, no row past the 128-edge floor
    of plan.hub_policy.  'hub': the same plus 300 edges into destination 11.  'small': 8 x 8, 300 edges (37 per row: column
    blocks allowed by both wide_blocks policies)."""
    rng = _rng(41000, 5)      # a draw of _graph without its own long row
    if name == "small":
        return rng.integers(0, 8, size=(2, 300)).astype(np.int32), 8
    ei = _graph(rng, N, N, 400)
    ei = ei[:, ei[0] != EMPTY_ROW]
    if name == "hub":
        long_row = np.stack([np.full(300, HUB_ROW, np.int32), _rng(41000, 4).integers(0, N, 300).astype(np.int32)])
        ei = np.concatenate([ei, long_row], 1)
    return ei, N


@pytest.fixture(scope="module")
def world(tfg):
    """The three plans and the operands every case shares (read-only)."""
    from tf_geometric_amd import plan as P
    L = tfg._lib
    w = {}
    for name in ("plain", "hub", "small"):
        ei, n = _edges(name)
        plan = P.CsrPlan.build(L.as_i32(ei), n, n)
        d = dict(ei=ei, n_dst=n, n_src=n, hub=None)
        indeg, _ = _degrees(ei, n, n)
        assert (plan.hub_info() is not None) == _hubs(d)[0] == (name == "hub"), name
        assert (plan.row_order() is not None) == _skewed(indeg, ei.shape[1]) == (name == "hub"), name
        assert (plan.hub_order_slot() is not None) == (name == "hub"), name
        if name != "small":
            assert indeg[EMPTY_ROW] == 0 and 650 <= ei.shape[1] + (300 if name == "plain" else 0) <= 750
        g = torch.Generator(device="cpu")
        g.manual_seed(41000 + len(name))
        E = ei.shape[1]
        w[name] = dict(plan=plan, n=n, E=E,
                       w=(torch.rand(E, generator=g) + 0.5).cuda(), self_coef=(torch.rand(n, generator=g) + 0.1).cuda(),
                       count=(torch.from_numpy(indeg.astype(np.int32)) + 1).cuda(), x={}, gen=g)
    return w


def _table(world, graph, kind, F):
    """The case's table, built once per (graph, kind, F): dense float32 (F = 20: a column block of a wider tensor, rows off
    the 16-byte boundary), a SplitRows with or without its per-edge tail, or a HalfRows on the stated stride."""
    from tf_geometric_amd import plan as P
    g = world[graph]
    key = (kind, F)
    if key not in g["x"]:
        n = g["n"]
        x32 = torch.randn(n, F, generator=g["gen"]).cuda()
        if kind == "f32":
            if F == 20:
                wide = _nan32((n, 23))
                wide[:, 1:21] = x32
                t = wide[:, 1:21]
            else:
                t = x32
        elif kind in ("split", "split_edge"):
            t = P.SplitRows.from_dense(x32)
            if kind == "split_edge":
                t.with_edge_tail(g["plan"])
        else:
            dtype = BF16 if kind == "bf16" else FP16
            ld = {20: 24, 100: 104}.get(F, P.h16_friendly_ld(F))
            table = _fill16((n, ld), dtype)
            table[:, :F] = x32.to(dtype)
            t = P.HalfRows(table, F)
        g["x"][key] = t
    return g["x"][key]


# --------------------------------------------------------------------------------------------------------------- the hand fill
def _hand_args(L, plan, table, keep, spans=None, w=None, n_dst=None, hub=False, order=False, slot=False):
    """A tfgx_reduce_args with the members every launch has: spans, col, w, n_dst, x / ldx / F (+ the split layout's), and —
    only where the caller says so — the walk order, the hub lists with a fresh scratch, hub_order_slot."""
    from tf_geometric_amd import plan as P
    a = L.ReduceArgs()
    if spans is None:
        a.row_begin, a.row_end, a.rp_stride, a.col = plan.row_ptr.data_ptr(), plan.row_ptr[1:].data_ptr(), 1, plan.col.data_ptr()
    else:
        rb, re, stride, col = spans[:4]
        a.row_begin, a.row_end, a.rp_stride, a.col = rb.data_ptr(), re.data_ptr(), stride, col.data_ptr()
    a.w = 0 if w is None else w.data_ptr()
    a.n_dst = plan.n_dst if n_dst is None else n_dst
    if isinstance(table, P.HalfRows):
        a.x, a.ldx, a.F = table.table.data_ptr(), table.ld, table.F
    elif isinstance(table, P.SplitRows):
        a.x, a.ldx, a.F = table.main.data_ptr(), int(table.main.stride(0)), table.shape[1]
        a.x_tail, a.ld_tail, a.f_main = table.tail.data_ptr(), int(table.tail.shape[1]), int(table.main.shape[1])
        if table.edge_tail is not None and spans is None:
            a.edge_tail, a.ld_edge_tail = table.edge_tail.data_ptr(), int(table.edge_tail.shape[1])
    else:
        a.x, a.ldx, a.F = table.data_ptr(), int(table.stride(0)), int(table.shape[1])
    if order:
        a.row_order = plan.row_order().data_ptr()
    if hub:
        rows, chunk_ptr, chunk_begin, chunk_end, _ = plan.hub_info()
        scratch = _nan32((int(chunk_begin.shape[0]), int(a.F)))
        keep.append(scratch)
        a.hub_threshold = plan.hub_threshold
        a.hub_rows, a.hub_chunk_ptr, a.hub_chunk_begin, a.hub_chunk_end = (t.data_ptr() for t in (rows, chunk_ptr, chunk_begin, chunk_end))
        a.n_hub_rows, a.n_hub_chunks, a.hub_scratch = int(rows.shape[0]), int(chunk_begin.shape[0]), scratch.data_ptr()
    if slot:
        a.hub_order_slot = plan.hub_order_slot().data_ptr()
    return a


class _Counters(object):
    """The launch counters of plan.py, and what a call moved them by."""
    NAMES = ("agg_launches", "fused", "fused_side", "fused_h16", "promotions", "served", "demotions")

    def __init__(self, P):
        self.P = P
        self.at = self.read()

    def read(self):
        P = self.P
        return (P._AGG_LAUNCHES[0], P.FUSED_STATS["launches"], P.FUSED_STATS["with_side_output"], P.FUSED_H16_STATS["launches"],
                P.VERIFIED_STATS["promotions"], P.VERIFIED_STATS["served"], P.VERIFIED_STATS["demotions"])

    def moved(self, **by):
        now = self.read()
        got = {k: b - a for k, a, b in zip(self.NAMES, self.at, now) if b != a}
        self.at = now
        assert got == {k: v for k, v in by.items() if v}, "counters moved by {}, expected {}".format(got, by)


# ------------------------------------------------------------------------------------------------------------- segment_reduce
def _seg(cid, graph, kind, F, op="sum", weighted=False, epi=False, add=False, count=False, mode=None, out=None, out_dtype=None,
         track=False, wide=None):
    return pytest.param(dict(graph=graph, kind=kind, F=F, op=op, weighted=weighted, epi=epi, add=add, count=count, mode=mode,
                             out=out, out_dtype=out_dtype, track=track, wide=wide), id=cid)


SEG_CASES = [
    # dense float32: unaligned rows at F = 20, every operand once, both graphs
    _seg("f32-20-hub-sum-w", "hub", "f32", 20, weighted=True),
    _seg("f32-20-plain-mean-count-epi-add", "plain", "f32", 20, op="mean", count=True, epi=True, add=True),
    _seg("f32-20-hub-max-out", "hub", "f32", 20, op="max", out="given"),
    _seg("f32-100-hub-sum-w-epi-add-out", "hub", "f32", 100, weighted=True, epi=True, add=True, out="given"),
    _seg("f32-100-hub-spans-mean-count-w-epi", "hub", "f32", 100, op="mean", count=True, weighted=True, epi=True, mode="spans"),
    _seg("f32-100-hub-n_dst", "hub", "f32", 100, weighted=True, mode="n_dst"),
    _seg("f32-128-hub-sum", "hub", "f32", 128, weighted=True, epi=True),
    _seg("f32-128-plain-max", "plain", "f32", 128, op="max"),
    _seg("f32-128-hub-track", "hub", "f32", 128, op="max", weighted=True, track=True),
    _seg("f32-128-plain-track", "plain", "f32", 128, op="max", track=True),
    _seg("f32-128-hub-track-spans", "hub", "f32", 128, op="max", track=True, mode="spans"),
    _seg("f32-256-small-wide+1", "small", "f32", 256, weighted=True, wide=1),
    _seg("f32-256-small-wide-1", "small", "f32", 256, op="mean", wide=-1),
    _seg("f32-256-small-hint", "small", "f32", 256, op="max"),
    # the split-row layout, with and without the per-edge tail
    _seg("split-100-hub-sum-w-epi", "hub", "split", 100, weighted=True, epi=True),
    _seg("split-100-plain-mean-count-add", "plain", "split", 100, op="mean", count=True, add=True),
    _seg("split_edge-100-hub-sum-w-out", "hub", "split_edge", 100, weighted=True, out="given"),
    _seg("split_edge-100-plain-max", "plain", "split_edge", 100, op="max"),
    _seg("split_edge-100-hub-spans", "hub", "split_edge", 100, weighted=True, mode="spans"),
    _seg("split-100-hub-n_dst", "hub", "split", 100, op="mean", mode="n_dst"),
    # 16-bit tables
    _seg("bf16-20-hub-sum-w-epi-add", "hub", "bf16", 20, weighted=True, epi=True, add=True),
    _seg("fp16-20-plain-mean-count", "plain", "fp16", 20, op="mean", count=True),
    _seg("bf16-100-hub-max-out", "hub", "bf16", 100, op="max", out="given"),
    _seg("fp16-100-hub-sum-w-out16", "hub", "fp16", 100, weighted=True, out="given", out_dtype=FP16),
    _seg("bf16-100-plain-out_dtype", "plain", "bf16", 100, weighted=True, epi=True, out_dtype=BF16),
    _seg("bf16-100-hub-out_dtype-f32", "hub", "bf16", 100, op="mean", out_dtype=torch.float32),
    _seg("bf16-100-hub-spans-mean-count-w-epi-add", "hub", "bf16", 100, op="mean", count=True, weighted=True, epi=True, add=True,
         mode="spans"),
    _seg("fp16-100-hub-n_dst", "hub", "fp16", 100, weighted=True, mode="n_dst"),
    _seg("bf16-128-hub-sum", "hub", "bf16", 128, weighted=True),
    _seg("fp16-128-plain-max-epi", "plain", "fp16", 128, op="max", epi=True),
    _seg("bf16-256-small-wide+1", "small", "bf16", 256, weighted=True, wide=1),
    _seg("fp16-256-small-wide-1", "small", "fp16", 256, op="mean", wide=-1),
    _seg("bf16-256-small-hint", "small", "bf16", 256, out_dtype=BF16),
]


@pytest.mark.parametrize("c", SEG_CASES)
def test_segment_reduce_equals_the_hand_filled_call(tfg, world, c):
    from tf_geometric_amd import plan as P
    L = tfg._lib
    lib = L.require_gpu()
    g = world[c["graph"]]
    plan, n, E, F = g["plan"], g["n"], g["E"], c["F"]
    table = _table(world, c["graph"], c["kind"], F)
    half = isinstance(table, P.HalfRows)
    op = {"sum": L.SUM, "mean": L.MEAN, "max": L.MAX}[c["op"]]
    gen = torch.Generator(device="cpu")
    gen.manual_seed(7)
    w = g["w"] if c["weighted"] else None
    epi = dict(self_coef=g["self_coef"], bias=torch.randn(F, generator=gen).cuda(), act=L.ACT_RELU) if c["epi"] else {}
    add = None
    if c["add"]:          # a column block of a wider tensor: ld_add != F
        add = torch.randn(n, F + 8, generator=gen).cuda()[:, 4:4 + F]
        assert add.stride(0) == F + 8
        epi["add_x"] = add
    if c["count"]:
        epi["mean_count"] = g["count"]
    n_run = n - 7 if c["mode"] == "n_dst" else n
    own = c["mode"] is None
    hub = own and c["graph"] == "hub" and not c["track"]
    order = own and c["graph"] == "hub" and F <= 128
    half_out = c["out_dtype"] in (BF16, FP16)
    xdt = L.H16_DTYPES[table.dtype] if half else None
    odt = L.H16_DTYPES[c["out_dtype"]] if half_out else L.DT_F32
    keep = []
    counters = _Counters(P)

    def new_out():
        """An output of the layout the Python entry allocates, or — out= given — one off the 16-byte boundary / on a wider stride."""
        given = c["out"] == "given"
        if half_out:
            return P.HalfRows(_fill16((n_run, P.h16_friendly_ld(F) + (8 if given else 0)), c["out_dtype"]), F)
        return _nan32((n_run, F + 3))[:, 1:1 + F] if (given and c["kind"] == "f32") else _nan32((n_run, F))

    def py_out():
        return new_out() if c["out"] == "given" else None

    def hand(spans, w_, op_, accumulate, last, out_t, track_t, describe):
        """One launch (or describe) at the C ABI; out_t: a float32 tensor or a HalfRows."""
        a = _hand_args(L, plan, table, keep, spans=spans, w=w_, n_dst=n_run, hub=hub, order=order)
        if isinstance(out_t, P.HalfRows):
            a.out, a.ldo = out_t.table.data_ptr(), out_t.ld
        else:
            a.out, a.ldo = out_t.data_ptr(), int(out_t.stride(0))
        a.op, a.accumulate = op_, 1 if accumulate else 0
        if last:
            if c["epi"]:
                a.act, a.self_coef, a.bias = L.ACT_RELU, epi["self_coef"].data_ptr(), epi["bias"].data_ptr()
            if add is not None:
                a.add_x, a.ld_add = add.data_ptr(), F + 8
            if c["count"]:
                a.mean_count = g["count"].data_ptr()
        if track_t is not None:
            a.track, a.ld_track = track_t.data_ptr(), int(track_t.stride(0))
            if spans is not None:
                a.track_row_begin = spans[4].data_ptr()
        if c["wide"] is not None:
            a.wide_blocks = c["wide"]
        elif half:
            a.wide_blocks = P.h16_wide_blocks_hint(spans is not None, hub, E, n_run)
        else:
            a.wide_blocks = P.wide_blocks_hint(spans is not None, hub, int(a.ldx), E, n_run)
        if describe:
            buf = ctypes.create_string_buffer(160)
            if half:
                L.check(lib.tfgx_segment_reduce_h16_describe(ctypes.byref(a), xdt, odt, buf, 160), "describe")
            else:
                L.check(lib.tfgx_segment_reduce_describe(ctypes.byref(a), buf, 160), "describe")
            return buf.value.decode()
        if half:
            L.check(lib.tfgx_segment_reduce_h16(ctypes.byref(a), xdt, odt, L.stream_ptr()), "tfgx_segment_reduce_h16")
        else:
            L.check(lib.tfgx_segment_reduce_f32(ctypes.byref(a), L.stream_ptr()), "tfgx_segment_reduce_f32")

    extra = {}
    if c["wide"] is not None:
        extra["wide_blocks"] = c["wide"]
    if c["out_dtype"] is not None:
        extra["out_dtype"] = c["out_dtype"]
    track_py = track_hand = None
    if c["track"]:
        track_py, track_hand = (torch.full((n_run, F), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        extra["track"] = track_py
    exp = new_out()

    if c["mode"] == "spans":
        # two chained launches over explicit sub-spans of every row (plan.source_blocks), the epilogue on the last one
        rpk, col_k = plan.source_blocks(2)
        wk = None if w is None else w.flip(0).contiguous()      # weights in col_k's order: any E values will do for identity
        out = py_out()
        if out is None:
            out = _nan32((n_run, F))
        for b in range(2):
            last = b == 1
            kw = dict(w_csr=wk, accumulate=b > 0, row_begin=rpk[b:], row_end=rpk[b + 1:], rp_stride=2, col=col_k, **extra)
            if c["track"]:
                kw["track_row_begin"] = rpk
            op_b = op if (last or op != L.MEAN) else L.SUM
            if last:
                kw.update(epi)
            spans = (rpk[b:], rpk[b + 1:], 2, col_k, rpk)
            name = P.segment_reduce(plan, table, op_b, out=out, describe=True, **kw)
            counters.moved()
            v0 = out._version
            got = P.segment_reduce(plan, table, op_b, out=out, **kw)
            counters.moved(agg_launches=1)
            assert got is out and out._version > v0
            assert name == hand(spans, wk, op_b, b > 0, last, exp, track_hand, True)
            hand(spans, wk, op_b, b > 0, last, exp, track_hand, False)
    else:
        kw = dict(w_csr=w, **dict(epi, **extra))
        if c["mode"] == "n_dst":
            kw["n_dst"] = n_run
        out = py_out()
        name = P.segment_reduce(plan, table, op, out=out, describe=True, **kw)
        counters.moved()
        v0 = (out._version, ) if isinstance(out, torch.Tensor) else None
        t0 = track_py._version if c["track"] else None
        got = P.segment_reduce(plan, table, op, out=out, **kw)
        counters.moved(agg_launches=1)
        if out is not None:
            assert got is out
            if v0 is not None:
                assert out._version > v0[0], "a caller's float32 out must have its version counter bumped"
        if c["track"]:
            assert track_py._version > t0
        assert name == hand(None, w, op, False, True, exp, track_hand, True)
        hand(None, w, op, False, True, exp, track_hand, False)
    torch.cuda.synchronize()
    if half_out:
        assert isinstance(got, P.HalfRows) and got.dtype == c["out_dtype"] and got.shape == (n_run, F)
        assert torch.equal(_bits16(got.table[:, :F]), _bits16(exp.table[:, :F]))
    else:
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (n_run, F)
        assert not bool(torch.isnan(exp).any()) and torch.equal(got, exp)
    if c["track"]:
        assert torch.equal(track_py, track_hand) and bool((track_py != -1).any())
    counters.moved()


# ------------------------------------------------------------------------------------------------------------- aggregate_gemm
def _gemm(cid, graph, kind, F, Nout, op="sum", weighted=False, epi=False, side=False, training=False, out=None):
    return pytest.param(dict(graph=graph, kind=kind, F=F, N=Nout, op=op, weighted=weighted, epi=epi, side=side, training=training,
                             out=out), id=cid)


GEMM_CASES = [
    _gemm("f32-100-hub-w-epi-side", "hub", "f32", 100, 64, weighted=True, epi=True, side=True),
    _gemm("f32-100-plain-mean", "plain", "f32", 100, 33, op="mean"),
    _gemm("f32-128-hub-N256-out", "hub", "f32", 128, 256, weighted=True, out="given"),
    _gemm("f32-128-plain-N256-side", "plain", "f32", 128, 256, op="mean", epi=True, side=True),
    _gemm("split-100-hub-w-side", "hub", "split", 100, 64, weighted=True, side=True),
    _gemm("split_edge-100-hub-w-epi", "hub", "split_edge", 100, 64, weighted=True, epi=True),
    _gemm("split_edge-100-plain-mean", "plain", "split_edge", 100, 64, op="mean", out="given"),
    _gemm("bf16-20-hub-w-epi", "hub", "bf16", 20, 16, weighted=True, epi=True),
    _gemm("fp16-100-hub-mean-side", "hub", "fp16", 100, 64, op="mean", side=True),
    _gemm("bf16-100-hub-training", "hub", "bf16", 100, 64, weighted=True, training=True),
    _gemm("bf16-100-plain-training-side-out", "plain", "bf16", 100, 33, weighted=True, epi=True, side=True, training=True, out="given"),
    _gemm("bf16-128-hub-N256", "hub", "bf16", 128, 256, weighted=True, epi=True),
    _gemm("fp16-128-plain-N256-side", "plain", "fp16", 128, 256, side=True),
]


@pytest.mark.parametrize("c", GEMM_CASES)
def test_aggregate_gemm_equals_the_hand_filled_call(tfg, world, c):
    from tf_geometric_amd import plan as P
    L = tfg._lib
    lib = L.require_gpu()
    g = world[c["graph"]]
    plan, n, F, Nout = g["plan"], g["n"], c["F"], c["N"]
    table = _table(world, c["graph"], c["kind"], F)
    half = isinstance(table, P.HalfRows)
    op = L.MEAN if c["op"] == "mean" else L.SUM
    gen = torch.Generator(device="cpu")
    gen.manual_seed(11)
    kernel = (torch.randn(F, Nout, generator=gen) / F ** 0.5).cuda()
    w = g["w"] if c["weighted"] else None
    sc, bias, act = (g["self_coef"], torch.randn(Nout, generator=gen).cuda(), L.ACT_RELU) if c["epi"] else (None, None, L.ACT_NONE)
    assert P.aggregate_gemm_applies(table, kernel, op) is True
    has_hub = c["graph"] == "hub"
    keep = []
    counters = _Counters(P)
    out = _nan32((n, Nout)) if c["out"] == "given" else None
    side = _nan32((n, F)) if c["side"] else None
    v0 = (None if out is None else out._version, None if side is None else side._version)
    got = P.aggregate_gemm(plan, table, op, kernel, w_csr=w, self_coef=sc, bias=bias, act=act, out=out, agg_out=side,
                           training=c["training"])
    counters.moved(agg_launches=1, fused=1, fused_side=1 if c["side"] else 0, fused_h16=1 if half else 0)
    assert got is not None and (out is None or (got is out and out._version > v0[0]))
    assert side is None or side._version > v0[1]

    a = _hand_args(L, plan, table, keep, w=w, hub=has_hub, order=has_hub, slot=has_hub)
    a.op = op
    a.self_coef = 0 if sc is None else sc.data_ptr()
    exp, exp_side = _nan32((n, Nout)), None
    if c["side"]:
        exp_side = _nan32((n, F))
        a.out, a.ldo = exp_side.data_ptr(), F
    if half:
        L.check(lib.tfgx_aggregate_gemm_h16(ctypes.byref(a), L.H16_DTYPES[table.dtype], L.ptr(kernel), Nout, L.ptr(bias), act,
                                            L.ptr(exp), Nout, Nout, L.stream_ptr()), "tfgx_aggregate_gemm_h16")
    else:
        L.check(lib.tfgx_aggregate_gemm_f32(ctypes.byref(a), L.ptr(kernel), Nout, L.ptr(bias), act, L.ptr(exp), Nout, Nout,
                                            L.stream_ptr()), "tfgx_aggregate_gemm_f32")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(exp).any()) and torch.equal(got, exp)
    if c["side"]:
        assert not bool(torch.isnan(exp_side).any()) and torch.equal(side, exp_side)
    counters.moved()


def test_aggregate_gemm_declines_without_counting(tfg, world, monkeypatch):
    """Outside tfgx_aggregate_gemm_fits (F = 256), a kernel of another height, MAX, and the switch: None, no counter moves."""
    from tf_geometric_amd import plan as P
    L = tfg._lib
    plan = world["small"]["plan"]
    counters = _Counters(P)
    for kind in ("f32", "bf16"):
        wide = _table(world, "small", kind, 256)
        assert P.aggregate_gemm(plan, wide, L.SUM, torch.zeros(256, 64, device="cuda")) is None
        assert P.aggregate_gemm_applies(wide, torch.zeros(256, 64, device="cuda")) is False
    for kind in ("f32", "split", "fp16"):
        t = _table(world, "hub", kind, 100)
        k = torch.zeros(100, 64, device="cuda")
        assert P.aggregate_gemm(world["hub"]["plan"], t, L.MAX, k) is None
        assert P.aggregate_gemm(world["hub"]["plan"], t, L.SUM, torch.zeros(96, 64, device="cuda")) is None
        monkeypatch.setattr(P, "FUSE_AGGREGATE_GEMM", False)
        assert P.aggregate_gemm(world["hub"]["plan"], t, L.SUM, k) is None and P.aggregate_gemm_applies(t, k) is False
        monkeypatch.setattr(P, "FUSE_AGGREGATE_GEMM", True)
    counters.moved()


def test_segment_reduce_refusals_keep_their_text(tfg, world):
    from tf_geometric_amd import plan as P
    L = tfg._lib
    plan = world["plain"]["plan"]
    x, h = _table(world, "plain", "f32", 100), _table(world, "plain", "bf16", 100)
    counters = _Counters(P)
    with pytest.raises(TypeError, match="^segment_reduce: out_dtype needs a HalfRows input$"):
        P.segment_reduce(plan, x, L.SUM, out_dtype=BF16)
    with pytest.raises(TypeError, match="^segment_reduce: out_dtype must be None, torch.float32, torch.bfloat16 or torch.float16$"):
        P.segment_reduce(plan, h, L.SUM, out_dtype=torch.float64)
    with pytest.raises(TypeError, match=r"^segment_reduce on a HalfRows: out must be a float32 \[n_dst, F\] tensor on the table's device "
                                        r"\(or a HalfRows with out_dtype=\)$"):
        P.segment_reduce(plan, h, L.SUM, out=torch.zeros(N, 100, dtype=torch.float64, device="cuda"))
    with pytest.raises(AssertionError, match="out must be a HalfRows of out_dtype"):
        P.segment_reduce(plan, h, L.SUM, out=torch.zeros(N, 100, device="cuda"), out_dtype=BF16)
    with pytest.raises(L.TfgxError, match=r"^tfgx_segment_reduce_h16: track: not supported on a 16-bit table \(max aggregation is "
                                          r"inference-only\)$"):
        P.segment_reduce(plan, h, L.MAX, track_row_begin=plan.row_ptr, out_dtype=torch.float64)      # before anything else
    assert P.segment_reduce(plan, x, L.SUM, out_dtype=torch.float32).dtype == torch.float32
    counters.moved(agg_launches=1)
