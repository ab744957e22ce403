# coding=utf-8
"""The dense GEMM and its weight gradient reading a 16-bit feature table (include/tfgx_gemm_h16.h), on the GPU.

The defining contract: plan.gemm_bias_act / plan.gemm_tn on a HalfRows return, BIT FOR BIT (torch.equal), what they return
for the table widened to float32 (h.float(): dense, lda = K) — on every route of the dispatcher (test_gemm_h16_abi.ROUTES:
each case first asserts through tfgx_gemm_describe that the float32 call takes the route it was built for), with bias / ReLU /
act_cols / a column-slice `out` / workspace lent or not, on both table strides, whatever the table's padding columns hold
(NaN patterns), and over non-finite and edge values.  The independent anchor — bit identity alone would pass if both routes
were wrong together — is float64 at assert_parity's default bar.  Then the layers that were refusing such a table: a table
declared a GEMM operand gives GCN / GAT / mean and sum GraphSAGE the float32 layer's bits on h.float(), outputs and every
parameter gradient, without a widened copy; an undeclared table is refused as before.

Mean / sum GraphSAGE on an UNDECLARED table: with units/2 >= F (aggregation first) both tables run the same launches apart
from the self half's A loads, so the layers agree bit for bit; with units/2 < F the declared table takes the float32 layer's
GEMM-first route while the undeclared one still aggregates first (today's behaviour, unchanged) — a re-association, held to
the 1e-5 bar tests/test_gpu_h16.py holds that layer to against the float32 layer."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import assert_parity
from test_gemm_h16_abi import ROUTES, roundup8

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
NAN_BITS = {torch.bfloat16: 0x7FC0, torch.float16: 0x7E00}
_RELU = 1


def _gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _lds(tfg, K):
    return sorted({roundup8(K), tfg.plan.h16_friendly_ld(K)})


_TABLES = {}


def _table(tfg, M, K, dtype, ld, pad_nan=False):
    """(HalfRows declared a GEMM operand, its widened dense float32 matrix); made once per (M, K, dtype, ld) and left unchanged."""
    key = (M, K, dtype, ld, pad_nan)
    if key not in _TABLES:
        x = torch.randn((M, K), generator=_gen(M * 31 + K), device="cuda")
        h = tfg.HalfRows.from_dense(x, dtype=dtype, ld=ld, gemm_operand=True)
        if pad_nan and ld > K:
            h.table.view(torch.int16)[:, K:] = int(NAN_BITS[dtype])
        _TABLES[key] = (h, h.float())
        if len(_TABLES) > 24:
            _TABLES.pop(next(iter(_TABLES)))
    return _TABLES[key]


def _weights(K, N, seed=0):
    g = _gen(1000 + 7 * K + N + seed)
    return (torch.randn((K, N), generator=g, device="cuda") * (0.5 / np.sqrt(K)),
            torch.randn(N, generator=g, device="cuda"))


def _route(tfg, a, W, out, M, K, N, lent):
    L = tfg._lib
    lib = L.load_library()
    buf = ctypes.create_string_buffer(200)
    wsb = lib.tfgx_gemm_workspace_bytes(M, K, N) if lent else 0
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device="cuda")
    L.check(lib.tfgx_gemm_describe(L.ptr(a), K, L.ptr(W), N, None, 0, 0, L.ptr(out), int(out.stride(0)) if M > 1 else N, M, K, N,
                                   L.ptr(ws) if wsb else None, wsb, buf, 200), "tfgx_gemm_describe")
    return buf.value.decode()


def _gemm(tfg, a, W, bias=None, act=0, act_cols=None, out=None, lend=True):
    """plan.gemm_bias_act, or the same C call without a workspace (lend=False)."""
    P, L = tfg.plan, tfg._lib
    if lend:
        return P.gemm_bias_act(a, W, bias=bias, act=act, out=out, act_cols=act_cols)
    lib = L.load_library()
    half = isinstance(a, P.HalfRows)
    M, K = a.shape
    N = int(W.shape[1])
    out = torch.empty((M, N), dtype=torch.float32, device="cuda") if out is None else out
    ldc = int(out.stride(0)) if M > 1 else N
    tail = (L.ptr(W), N, L.ptr(bias), act, N if act_cols is None else act_cols, L.ptr(out), ldc, M, K, N, None, 0, L.stream_ptr())
    if half:
        L.check(lib.tfgx_gemm_bias_act_cols_ws_h16(L.ptr(a.table), L.H16_DTYPES[a.dtype], a.ld, *tail), "h16")
    else:
        L.check(lib.tfgx_gemm_bias_act_cols_ws_f32(L.ptr(a), K, *tail), "f32")
    return out


def _variants(N):
    """bias / ReLU / partial act_cols / out a column slice of a wider tensor / workspace not lent"""
    return [dict(), dict(bias=True, act=_RELU), dict(bias=True, act=_RELU, act_cols=N // 2), dict(slice=True, bias=True),
            dict(lend=False, act=_RELU)]


def _run(tfg, a, W, b, M, N, v):
    out = None
    if v.get("slice"):
        wide = torch.full((M, N + 12), -7.0, device="cuda")
        out = wide[:, 4:4 + N]
    got = _gemm(tfg, a, W, bias=b if v.get("bias") else None, act=v.get("act", 0), act_cols=v.get("act_cols"), out=out,
                lend=v.get("lend", True))
    if v.get("slice"):
        assert bool((wide[:, :4] == -7.0).all()) and bool((wide[:, 4 + N:] == -7.0).all()), "wrote outside its column slice"
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", ROUTES, ids=["{}x{}to{}{}".format(m, k, n, "ws" if w else "") for m, k, n, w, _ in ROUTES])
def test_forward_equals_the_float32_route_bit_for_bit(tfg, case, dtype):
    M, K, N, lent, pattern = case
    W, b = _weights(K, N)
    for ld in _lds(tfg, K):
        h, xf = _table(tfg, M, K, dtype, ld)
        assert h.ld == ld and xf.is_contiguous() and xf.data_ptr() % 16 == 0
        route = _route(tfg, xf, W, torch.empty((M, N), device="cuda"), M, K, N, lent)
        assert re.fullmatch(pattern, route), (case[:4], route)
        for v in _variants(N):
            if lent and not v.get("lend", True):
                continue                                   # the case is about the workspace route
            got, ref = _run(tfg, h, W, b, M, N, v), _run(tfg, xf, W, b, M, N, v)
            assert got.dtype == torch.float32 and torch.equal(got, ref), (case[:4], str(dtype), ld, v)


PAD_CASES = [(32805, 36, 40), (32805, 65, 7), (32805, 1433, 16), (37, 7, 5), (32805, 101, 256)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", PAD_CASES, ids=["rows36", "skinny65", "skinny1433", "generic7", "generic101"])
def test_padding_columns_never_reach_a_result(tfg, shape, dtype):
    """Every padding column [K, ld) holds the NaN pattern; one shape per kernel whose K is no multiple of its step."""
    M, K, N = shape
    W, b = _weights(K, N)
    for ld in {roundup8(K) if roundup8(K) > K else K + 8, tfg.plan.h16_friendly_ld(K) if tfg.plan.h16_friendly_ld(K) > K else K + 8}:
        h, xf = _table(tfg, M, K, dtype, ld, pad_nan=True)
        assert ld > K and bool(torch.isnan(h.table[:, K:].float()).all())
        for v in (dict(), dict(bias=True, act=_RELU), dict(lend=False)):
            got, ref = _run(tfg, h, W, b, M, N, v), _run(tfg, xf, W, b, M, N, v)
            assert not bool(torch.isnan(ref).any()) and torch.equal(got, ref), (shape, str(dtype), ld, v)
        # the weight gradient reads the same table
        g = torch.randn((M, N), generator=_gen(5), device="cuda")
        dW, db = tfg.plan.gemm_tn(h, g, want_bias=True)
        rW, rb = tfg.plan.gemm_tn(xf, g, want_bias=True)
        assert torch.equal(dW, rW) and torch.equal(db, rb) and not bool(torch.isnan(rW).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", [(32805, 100, 47), (32805, 602, 16), (513, 100, 47), (32805, 1433, 64)],
                         ids=["rows", "skinny", "generic_short", "generic_long"])
def test_non_finite_and_edge_values(tfg, shape, dtype):
    """+-inf, NaN, -0, fp16 subnormals and the largest finite values in the table: equal after nan_to_num, NaNs in the same places."""
    M, K, N = shape
    x = torch.randn((M, K), generator=_gen(77), device="cuda")
    top = float(torch.finfo(dtype).max)
    specials = torch.tensor([float("inf"), -float("inf"), float("nan"), -0.0, 6.0e-8, -3.0e-6, top, -top], device="cuda")
    idx = torch.randint(0, M * K, (M // 4,), generator=_gen(78), device="cuda")
    x.view(-1)[idx] = specials[torch.arange(idx.numel(), device="cuda") % specials.numel()]
    h = tfg.HalfRows.from_dense(x, dtype=dtype, gemm_operand=True)
    xf = h.float()
    assert bool(torch.isnan(xf).any()) and bool(torch.isinf(xf).any())
    W, b = _weights(K, N)
    for v in (dict(), dict(bias=True, act=_RELU)):
        got, ref = _run(tfg, h, W, b, M, N, v), _run(tfg, xf, W, b, M, N, v)
        assert torch.equal(torch.isnan(got), torch.isnan(ref))
        assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(ref, nan=0.0))
        assert bool(torch.isnan(ref).any()) and not bool(torch.isnan(ref).all())
    g = torch.randn((M, N), generator=_gen(79), device="cuda")
    dW, db = tfg.plan.gemm_tn(h, g, want_bias=True)
    rW, rb = tfg.plan.gemm_tn(xf, g, want_bias=True)
    assert torch.equal(torch.isnan(dW), torch.isnan(rW)) and torch.equal(torch.nan_to_num(dW, nan=0.0), torch.nan_to_num(rW, nan=0.0))
    assert torch.equal(db, rb)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", [(32805, 100, 47), (32805, 602, 16)], ids=["rows", "skinny"])
def test_forward_against_float64(tfg, shape, dtype):
    M, K, N = shape
    W, b = _weights(K, N)
    h, xf = _table(tfg, M, K, dtype, tfg.plan.h16_friendly_ld(K))
    got = tfg.plan.gemm_bias_act(h, W, bias=b)
    ref = xf.double() @ W.double() + b.double()
    assert_parity(got.cpu().numpy(), ref.cpu().numpy(), what="h16 GEMM {} vs float64".format(shape))
    dW, db = tfg.plan.gemm_tn(h, got, want_bias=True)
    scale = float(np.sqrt(M))          # sums of M terms of order 1: float32 rounding grows like sqrt(M), so the bar is applied per sqrt(M)
    assert_parity((dW / scale).cpu().numpy(), ((xf.double().t() @ got.double()) / scale).cpu().numpy(), what="h16 gemm_tn dW")
    assert_parity((db / scale).cpu().numpy(), (got.double().sum(0) / scale).cpu().numpy(), what="h16 gemm_tn db")


TN_CASES = [(37, 7, 5), (32805, 100, 47), (32805, 100, 256), (32805, 256, 40), (32805, 602, 16), (2708, 1433, 16),
            (524291, 128, 128), (0, 100, 16)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", TN_CASES, ids=["{}x{}to{}".format(*s) for s in TN_CASES])
def test_weight_gradient_equals_the_float32_route_bit_for_bit(tfg, shape, dtype):
    M, K, N = shape
    P = tfg.plan
    if M == 0:
        h = P.HalfRows(torch.empty((0, P.h16_friendly_ld(K)), dtype=dtype, device="cuda"), K, gemm_operand=True)
        g = torch.empty((0, N), device="cuda")
        for want_bias in (False, True):
            dW, db = P.gemm_tn(h, g, want_bias=want_bias)
            assert dW.shape == (K, N) and not bool(dW.any()) and (db is None) == (not want_bias) and (db is None or not bool(db.any()))
        return
    big = M * N >= 1 << 26                     # the column-sum split: M N >= 2^26, Ka % 16 == 0, with bias
    g = torch.randn((M, N), generator=_gen(3), device="cuda")
    gate = torch.randn((M, N), generator=_gen(4), device="cuda")
    for ld in (_lds(tfg, K)[-1:] if big else _lds(tfg, K)):
        h, xf = _table(tfg, M, K, dtype, ld)
        for want_bias in ((True,) if big else (False, True)):
            for gt in ((None,) if big else (None, gate)):
                dW, db = P.gemm_tn(h, g, want_bias=want_bias, gate=gt)
                rW, rb = P.gemm_tn(xf, g, want_bias=want_bias, gate=gt)
                assert torch.equal(dW, rW), (shape, str(dtype), ld, want_bias, gt is not None)
                assert (db is None and rb is None) or torch.equal(db, rb), (shape, str(dtype), ld, want_bias, gt is not None)
                assert bool(rW.any())
    if big:
        assert tfg._lib.load_library().tfgx_gemm_tn_workspace_bytes(M, K, N, 1) > tfg._lib.load_library().tfgx_gemm_tn_workspace_bytes(M, K, N, 0)


# ---------------------------------------------------------------------------------------------------------------- layers
_GRAPHS = {}


def _graph(tfg, n):
    if n not in _GRAPHS:
        rng = np.random.default_rng(n)
        ei = tfg._lib.as_i32(rng.integers(0, n, size=(2, 8 * n)).astype(np.int32))
        w = tfg._lib.as_f32(rng.uniform(0.2, 1.5, size=8 * n).astype(np.float32))
        _GRAPHS[n] = (ei, w)
    return _GRAPHS[n]


def _layer_makers(tfg, F):
    ly = tfg.layers
    out = [("GCN16", lambda: ly.GCN(16, activation=tfg.relu), False), ("GAT16", lambda: ly.GAT(16), False),
           ("GAT64x8", lambda: ly.GAT(64, num_heads=8), False)]
    for cls in (ly.MeanGraphSage, ly.SumGraphSage):
        for concat in (True, False):
            units = 64 if concat else 32                 # units/2 < F (concat) / units < F: the GEMM-first route
            out.append(("{}{}".format(cls.__name__, "cat" if concat else "add"), lambda c=cls, u=units, k=concat: c(u, concat=k), True))
    return out


def _build(tfg, make, x, ei, w, weighted):
    layer = make()
    with torch.no_grad():
        layer([x, ei, w] if weighted else [x, ei])       # lazy build
        for p in layer.parameters():
            if p.dim() == 1:
                p.uniform_(-0.1, 0.1, generator=_gen(11))
    return layer


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("n,F", [(3000, 100), (3000, 1433), (40000, 100), (40000, 1433)])
def test_layers_on_a_declared_table_equal_the_float32_layers(tfg, n, F, dtype):
    ei, w = _graph(tfg, n)
    x = torch.randn((n, F), generator=_gen(n + F), device="cuda")
    h = tfg.prepare_half_features(x, dtype, gemm_operand=True)
    assert h.gemm_operand
    xf = h.float()
    t = xf.to(dtype)                                     # the same values as a 16-bit tensor that wants a gradient
    for name, make, weighted in _layer_makers(tfg, F):
        inputs = (lambda a: [a, ei, w]) if weighted else (lambda a: [a, ei])
        layer = _build(tfg, make, xf, ei, w, weighted)
        with torch.no_grad():
            a, b = layer(inputs(h)), layer(inputs(xf))
        assert torch.equal(a, b), (name, "inference")
        layer.trainable(True)
        gout = torch.randn(a.shape, generator=_gen(5), device="cuda")
        grads = []
        for src in (h, xf):
            for p in layer.parameters():
                p.grad = None
            out = layer(inputs(src))
            out.backward(gout)
            grads.append((out.detach(), [p.grad.clone() for p in layer.parameters()]))
        assert torch.equal(grads[0][0], grads[1][0]), (name, "training forward")
        assert len(grads[0][1]) >= 2
        for ga, gb in zip(*[g[1] for g in grads]):
            assert torch.equal(ga, gb) and bool(gb.any()), (name, "parameter gradient")
        # d/dx reaches the 16-bit source: the float32 route's d/dx rounded to its dtype
        t16 = t.clone().requires_grad_(True)
        x32 = xf.clone().requires_grad_(True)
        layer(inputs(tfg.HalfRows.from_tensor(t16, gemm_operand=True))).backward(gout)
        layer(inputs(x32)).backward(gout)
        assert t16.grad is not None and t16.grad.dtype == dtype and torch.equal(t16.grad, x32.grad.to(dtype)), (name, "d/dx")
        layer.trainable(False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_no_widened_copy(tfg, dtype):
    """Around the forward of GCN(16) on the declared 40000 x 1433 table the allocation peak rises by less than half of 4 N F
    bytes (a widened copy alone is 4 N F)."""
    n, F = 40000, 1433
    ei, _ = _graph(tfg, n)
    h = tfg.prepare_half_features(torch.randn((n, F), generator=_gen(1), device="cuda"), dtype, gemm_operand=True)
    layer = tfg.layers.GCN(16)
    cache = {}
    with torch.no_grad():
        layer([h, ei], cache=cache)                      # builds the weights, the plan and the normalised adjacency
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        layer([h, ei], cache=cache)
        torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert rise < 4 * n * F // 2, "peak rose by {} bytes; a widened copy is {}".format(rise, 4 * n * F)


def test_undeclared_table(tfg):
    """gemm_operand=False: GCN / GAT refuse as before; mean / sum GraphSAGE behave as before — and agree with the declared table
    (bit for bit where both aggregate first, at the 1e-5 bar where the declared one takes the GEMM-first route)."""
    n, F = 3000, 100
    ei, w = _graph(tfg, n)
    x = torch.randn((n, F), generator=_gen(9), device="cuda")
    plain = tfg.prepare_half_features(x, torch.bfloat16)
    flagged = tfg.prepare_half_features(x, torch.bfloat16, gemm_operand=True)
    assert not plain.gemm_operand and torch.equal(plain.table[:, :F], flagged.table[:, :F])      # (padding columns are undefined)
    with pytest.raises(TypeError, match="before aggregating"):
        tfg.layers.GCN(16)([plain, ei])
    with pytest.raises(TypeError, match="before aggregating"):
        tfg.layers.GAT(16)([plain, ei])
    for cls in (tfg.layers.MeanGraphSage, tfg.layers.SumGraphSage):
        for units, same_route in ((256, True), (64, False)):
            layer = cls(units)
            with torch.no_grad():
                a, b, c = layer([plain, ei, w]), layer([flagged, ei, w]), layer([flagged.float(), ei, w])
            assert torch.equal(b, c), (cls.__name__, units)
            if same_route:
                assert torch.equal(a, b), (cls.__name__, units)
            else:
                assert_parity(a.cpu().numpy(), b.cpu().numpy(), tol=1e-5, what="{}({}) undeclared vs declared".format(cls.__name__, units))
            # training: the wide route's parameter gradients agree bit for bit as well
            if same_route:
                layer.trainable(True)
                gout = torch.randn(a.shape, generator=_gen(6), device="cuda")
                got = []
                for src in (plain, flagged):
                    for p in layer.parameters():
                        p.grad = None
                    layer([src, ei, w]).backward(gout)
                    got.append([p.grad.clone() for p in layer.parameters()])
                for ga, gb in zip(*got):
                    assert torch.equal(ga, gb)
