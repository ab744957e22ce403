# coding=utf-8
"""16-bit feature tables (include/tfgx_h16.h, plan.HalfRows) on the GPU.

The defining contract: a reduce over a 16-bit table returns, BIT FOR BIT, what the float32 route returns for that table
widened to float32 with the same plan structures (torch.equal).  The independent anchor — bit identity alone would pass if
both routes shared a bug — is float64 numpy on the widened table at the project's bar, 1e-5 * sqrt(max column sum of
|messages|) through assert_parity (MAX: bit for bit), as test_gpu_fuzz_forward._check_values.  Draws: test_h16_abi.draw_h16
(its census asserts without a device that the default seeds reach every instantiation)."""
import numpy as np
import pytest
import torch

from conftest import assert_parity
from test_gpu_fuzz_backward import _degrees, _hubs, _rng, _skewed
from test_gpu_fuzz_forward import _check_values, _desc, _partition, _segment_reference
from test_h16_abi import BF16, N_H16, _SCALE, _target_of, draw_h16, h16_kernel_name

pytestmark = pytest.mark.gpu
_TORCH_DT = {BF16: torch.bfloat16, 2: torch.float16}
_FILL16 = 0x7FFF          # a NaN in both 16-bit formats (as int16)


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _nan32(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _still_nan32(t):
    return bool((t.contiguous().view(torch.int32) == 0x7FC00000).all())


def _fill16(shape, dtype):
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return torch.full(shape, _FILL16, dtype=torch.int16, device="cuda").view(dtype)


def _same16(got, ref, what):
    """int16 bit patterns equal wherever the reference is not NaN; NaN-ness equal everywhere."""
    gn, rn = torch.isnan(got.float()), torch.isnan(ref.float())
    assert torch.equal(gn, rn), what + ": NaN-ness differs"
    same = (_bits16(got) == _bits16(ref)) | rn
    assert bool(same.all()), "{}: {} elements differ".format(what, int((~same).sum()))


# ------------------------------------------------------------------------------------------------------------- 1. converters
def _converter_inputs(rng, n, F):
    x = (rng.standard_normal((n, F)) * np.exp2(rng.uniform(-140, 127, size=(n, F)))).astype(np.float32)
    flat = x.reshape(-1)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 65504.0, 65519.9, 65520.0, 70000.0, -1e38, 3.4e38,      # fp16 overflow
                        1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,               # rounding ties
                        2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25, 6e-8, 1e-45, 2.0 ** -133,  # subnormals
                        2.0 ** -126 * (1 + 2.0 ** -8)], np.float32)
    k = min(flat.shape[0], special.shape[0])
    flat[rng.choice(flat.shape[0], k, replace=False)] = special[:k]
    return x


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,F,ld_src,ld_dst,off", [(37, 100, 100, 104, 0), (64, 128, 132, 128, 0), (5, 7, 9, 11, 1), (33, 47, 47, 64, 0),
                                                   (1, 1, 1, 8, 0), (19, 256, 256, 320, 3)])
def test_converters_against_torch(tfg, dtype, n, F, ld_src, ld_dst, off):
    """tfgx_rows_f32_to_h16 against tensor.cpu().to(dtype) and tfgx_rows_h16_to_f32 back, as int16 / int32 bits; a NaN-filled
    destination keeps its fill in columns [F, ld) and in rows >= n."""
    L = tfg._lib
    lib = L.require_gpu()
    dt = L.H16_DTYPES[dtype]
    rng = _rng(20000, n * 1000 + F)
    x = _converter_inputs(rng, n, F)
    src = _nan32((n, ld_src))
    src[:, :F] = torch.from_numpy(x).cuda()
    dst = _fill16((n + 2) * ld_dst + off, dtype)
    L.check(lib.tfgx_rows_f32_to_h16(L.ptr(src), ld_src, n, F, dst.data_ptr() + 2 * off, ld_dst, dt, L.stream_ptr()), "to_h16")
    body = dst[off:off + (n + 2) * ld_dst - off].reshape(-1)[:(n + 1) * ld_dst].reshape(n + 1, ld_dst)
    ref = torch.from_numpy(x).to(dtype).cuda()
    _same16(body[:n, :F], ref, "f32 -> {}".format(dtype))
    assert bool((_bits16(body[:n, F:]) == _FILL16).all()) and bool((_bits16(body[n:]) == _FILL16).all()), "padding was written"
    assert bool((_bits16(dst[:off]) == _FILL16).all())
    back = _nan32((n + 1, ld_src))
    L.check(lib.tfgx_rows_h16_to_f32(dst.data_ptr() + 2 * off, ld_dst, dt, n, F, L.ptr(back), ld_src, L.stream_ptr()), "to_f32")
    wide = ref.float()
    nan = torch.isnan(wide)
    assert torch.equal(torch.isnan(back[:n, :F]), nan)
    assert bool(((back[:n, :F].contiguous().view(torch.int32) == wide.contiguous().view(torch.int32)) | nan).all()), "widening is not exact"
    assert _still_nan32(back[:n, F:]) and _still_nan32(back[n:])
    # the Python entry points: friendly stride, same bits
    h = tfg.prepare_half_features(torch.from_numpy(x), dtype=dtype)
    assert h.shape == (n, F) and h.dtype == dtype and h.ld == lib.tfgx_h16_friendly_ld(F)
    _same16(h.table[:, :F], ref, "prepare_half_features")
    f = tfg.half_features_to_f32(h)
    assert f.shape == (n, F) and f.dtype == torch.float32 and bool(((f.view(torch.int32) == wide.view(torch.int32)) | nan).all())


# ------------------------------------------------------------------------------------------------------ 2. / 3. bit identity
@pytest.mark.parametrize("seed", range(N_H16 * _SCALE))
def test_fuzz_h16_bit_identity(tfg, seed):
    """segment_reduce(plan, H, ...) == segment_reduce(plan, H.float(), ...) with torch.equal over the argument surface; both
    held to float64 on the widened table; outputs inside NaN-filled wider buffers; a 16-bit output == result.to(dtype)."""
    from tf_geometric_amd import plan as P
    L = tfg._lib
    d = draw_h16(seed)
    what = "fuzz h16 " + _desc(d)
    rng = _rng(21500, seed)
    F, n_src, n_dst, ei, s, ldx = d["F"], d["n_src"], d["n_dst"], d["ei"], d["setting"], d["ldx"]
    dtype = _TORCH_DT[d["dt"]]
    E = ei.shape[1]
    x32 = rng.standard_normal((n_src, F)).astype(np.float32)
    if d["quant"]:
        x32 = np.round(x32 * 2) / 2 + np.float32(0)
    w = None
    if d["weighted"]:
        w = (rng.integers(1, 4, size=E) * 0.5).astype(np.float32) if d["quant"] else rng.uniform(-1.5, 1.5, size=E).astype(np.float32)
    sc = rng.uniform(0.1, 1.0, size=n_dst).astype(np.float32) if d["self"] else None
    bias = rng.standard_normal(F).astype(np.float32) if d["bias"] else None
    deg = np.bincount(ei[0], minlength=n_dst)
    count = deg + (rng.integers(0, 4, size=n_dst) if d["count_extra"] else 0)
    old = P.HUB_THRESHOLD, P.HUB_CHUNK, P.USE_ROW_ORDER
    try:
        if d["hub"]:
            P.HUB_THRESHOLD, P.HUB_CHUNK = d["hub"]
        plan = P.CsrPlan.build(L.as_i32(ei), n_dst, n_src)
        indeg, _ = _degrees(ei, n_dst, n_src)
        assert (plan.hub_info() is not None) == _hubs(d)[0], what
        assert (plan.row_order() is not None) == _skewed(indeg, E), what
        # the 16-bit table: torch's own rounding on the host, pad columns NaN; the widened table is what both routes stand for
        table = _fill16((n_src, ldx), dtype)
        table[:, :F] = torch.from_numpy(x32).to(dtype).cuda()
        H = P.HalfRows(table, F)
        xf = H.float()
        assert torch.equal(xf, table[:, :F].float()), what + ": HalfRows.float() != torch's widening"
        x = xf.cpu().numpy()
        wd = None if w is None else plan.edge_attr_to_csr(w)
        n_run = d["n_run"]
        spans = s == "spans"
        epi = dict(self_coef=None if sc is None else L.as_f32(sc), bias=None if bias is None else L.as_f32(bias),
                   add_x=xf if d["add_x"] else None, act=L.ACT_RELU if d["relu"] else L.ACT_NONE)
        cnt_d = L.as_i32(count) if (d["op"] == 1 and (d["count_extra"] or spans)) else None
        P.USE_ROW_ORDER = d["row_order"]

        def buffers():
            wide_out = _nan32((n_dst, F + d["out_off"] + d["out_pad"]))
            return wide_out, wide_out[:, d["out_off"]:d["out_off"] + F]

        def run(xin, primary=False):
            """The draw's launches on one route: xin = H (16-bit kernel) or xf (float32 kernel)."""
            half = xin is H
            wide_out, out = buffers()
            extra = dict(wide_blocks=d["wide_blocks"]) if half else {}
            if half:
                name = P.segment_reduce(plan, xin, d["op"], out=out, describe=True, w_csr=wd, **extra)
                assert name == h16_kernel_name(d["dt"], F, ldx, table.data_ptr(), d["op"] == 2, w is not None, d["wide_blocks"]), what
                assert not primary or _target_of(name) == d["target"], what + ": ran " + name
            else:
                assert P.segment_reduce(plan, xin, d["op"], out=out, describe=True, w_csr=wd).startswith("seg_reduce_kernel<"), what
            if spans:
                k1 = d["k1"]
                rpk_t, col_k = plan.source_blocks(k1)
                rp, col = plan.row_ptr.cpu().numpy().astype(np.int64), plan.col.cpu().numpy().astype(np.int64)
                _, order = _partition(rp, col, n_src, k1)
                wk = None if wd is None else L.as_f32(wd.cpu().numpy()[order])
                for b in range(k1):
                    kw = dict(w_csr=wk, accumulate=b > 0, row_begin=rpk_t[b:], row_end=rpk_t[b + 1:], rp_stride=k1, col=col_k, **extra)
                    if b == k1 - 1:
                        P.segment_reduce(plan, xin, d["op"], out=out, mean_count=cnt_d, **dict(kw, **epi))
                    else:
                        P.segment_reduce(plan, xin, L.SUM if d["op"] == 1 else d["op"], out=out, **kw)
            else:
                kw = dict(w_csr=wd, mean_count=cnt_d, **epi)
                if s == "n_dst":
                    kw["n_dst"] = n_run
                P.segment_reduce(plan, xin, d["op"], out=out, **dict(kw, **extra))
            return wide_out, out, (dict(kw) if not spans else None)

        wide_h, got, kw = run(H, primary=True)
        wide_f, exp, _ = run(xf)
        assert torch.equal(got[:n_run], exp[:n_run]), "{}: 16-bit route != float32 route on the widened table ({} elements)".format(
            what, int((got[:n_run].contiguous().view(torch.int32) != exp[:n_run].contiguous().view(torch.int32)).sum()))
        ref, scale = _segment_reference(d, x, w, ei, sc, bias, count, n_run)
        _check_values(d, got[:n_run], ref, scale, what + " [h16 vs float64]")
        _check_values(d, exp[:n_run], ref, scale, what + " [f32 vs float64]")
        if n_run < n_dst:
            assert _still_nan32(got[n_run:]), what + ": rows past n_dst were written"
        if d["out_off"] or d["out_pad"]:
            assert _still_nan32(wide_h[:, :d["out_off"]]) and _still_nan32(wide_h[:, d["out_off"] + F:]), what + ": columns outside the block"
        if spans:
            return
        first = got.clone()
        # run to run; walk order on = off; column blocks = one burst per row
        P.USE_ROW_ORDER = not d["row_order"]
        _, again, _ = run(H)
        assert torch.equal(again[:n_run], first[:n_run]), what + ": row order on != off"
        P.USE_ROW_ORDER = d["row_order"]
        _, again, _ = run(H)
        assert torch.equal(again[:n_run], first[:n_run]), what + ": run to run"
        if d["wide_blocks"] > 0:
            burst = P.segment_reduce(plan, H, d["op"], out=_nan32((n_dst, F)), **dict(kw, wide_blocks=-1))
            assert torch.equal(burst[:n_run], first[:n_run]), what + ": wide_blocks +1 != -1"
        if d["half_out"]:
            # 16-bit output on a NaN-filled table: == float32 result rounded by torch, the fill kept everywhere else
            for ld_o in (P.h16_friendly_ld(F), (F + 7) // 8 * 8 + 8 * d["out_pad"]):
                o = P.HalfRows(_fill16((n_dst, ld_o), dtype), F)
                r = P.segment_reduce(plan, H, d["op"], out=o, out_dtype=dtype, **dict(kw, wide_blocks=d["wide_blocks"]))
                assert r is o
                _same16(o.table[:n_run, :F], first[:n_run].to(dtype), what + ": 16-bit output")
                assert bool((_bits16(o.table[:, F:]) == _FILL16).all()) and bool((_bits16(o.table[n_run:]) == _FILL16).all()), \
                    what + ": 16-bit output wrote outside the launch"
    finally:
        P.HUB_THRESHOLD, P.HUB_CHUNK, P.USE_ROW_ORDER = old


def test_h16_refusals_reach_python(tfg):
    from tf_geometric_amd import plan as P
    L = tfg._lib
    ei = np.array([[0, 1, 2, 2], [1, 2, 0, 1]], np.int32)
    plan = P.CsrPlan.build(L.as_i32(ei), 3, 3)
    h = tfg.prepare_half_features(torch.randn(3, 32))
    with pytest.raises(L.TfgxError, match="accumulate"):
        P.segment_reduce(plan, h, L.SUM, accumulate=True, out_dtype=torch.bfloat16)
    with pytest.raises(L.TfgxError, match="track"):
        P.segment_reduce(plan, h, L.MAX, track=torch.zeros(3, 32, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        P.HalfRows(torch.zeros(3, 12, dtype=torch.bfloat16, device="cuda"), 12)


# ------------------------------------------------------------------------------------------------------- 4. no behaviour change
def test_plain_16_bit_tensor_still_takes_the_float32_kernel(tfg, monkeypatch):
    """A plain torch.bfloat16 tensor through the public entry that widens it (aggregate_neighbors -> _lib.as_f32): the 16-bit
    launch is never reached, the result is the float32 route's, and what the entry hands down names seg_reduce_kernel<."""
    from tf_geometric_amd import plan as P
    L = tfg._lib
    rng = _rng(22000, 0)
    ei = rng.integers(0, 50, size=(2, 600)).astype(np.int32)
    plan = P.CsrPlan.build(L.as_i32(ei), 50, 50)
    xb = torch.randn(50, 64, device="cuda").to(torch.bfloat16)
    half_launches = []
    lib = L.require_gpu()
    real = lib.tfgx_segment_reduce_h16      # counted at the library entry: whatever Python path leads there
    monkeypatch.setattr(lib, "tfgx_segment_reduce_h16", lambda *a: (half_launches.append(1), real(*a))[1])
    a = tfg.nn.aggregate_neighbors(xb, L.as_i32(ei), updater=tfg.nn.identity_updater)
    assert not half_launches, "a plain 16-bit tensor reached tfgx_segment_reduce_h16"
    b = tfg.nn.aggregate_neighbors(xb.float(), L.as_i32(ei), updater=tfg.nn.identity_updater)
    assert a.dtype == torch.float32 and torch.equal(a, b)
    widened = L.as_f32(xb)
    assert widened.dtype == torch.float32 and torch.equal(widened, xb.float())
    assert P.segment_reduce(plan, widened, L.SUM, describe=True).startswith("seg_reduce_kernel<")
    assert torch.equal(P.segment_reduce(plan, widened, L.SUM), P.segment_reduce(plan, P.HalfRows.from_tensor(xb), L.SUM))
    assert half_launches, "the opt-in HalfRows did not reach tfgx_segment_reduce_h16"


# -------------------------------------------------------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mean", [False, True])
def test_h16_autograd_matches_the_float32_route(tfg, dtype, mean):
    from tf_geometric_amd import autograd as AG
    from tf_geometric_amd import plan as P
    L = tfg._lib
    rng = _rng(23000, int(mean))
    n, F, E = 120, 100, 1500
    ei = rng.integers(0, n, size=(2, E)).astype(np.int32)
    plan = P.CsrPlan.build(L.as_i32(ei), n, n)
    op = L.MEAN if mean else L.SUM
    w = L.as_f32(rng.uniform(0.2, 1.5, size=E).astype(np.float32))
    w_csr = plan.edge_attr_to_csr(w)
    sc = L.as_f32(rng.uniform(0.1, 1.0, size=n).astype(np.float32))
    t = torch.randn(n, F, device="cuda").to(dtype).requires_grad_(True)
    bias_h = torch.randn(F, device="cuda").requires_grad_(True)
    gout = torch.randn(n, F, device="cuda")
    out_h = AG.aggregate(plan, P.HalfRows.from_tensor(t), op, w_csr, sc, bias=bias_h, act=L.ACT_RELU)
    out_h.backward(gout)
    xf = t.detach().float().requires_grad_(True)
    bias_f = bias_h.detach().clone().requires_grad_(True)
    out_f = AG.aggregate(plan, xf, op, w_csr, sc, bias=bias_f, act=L.ACT_RELU)
    out_f.backward(gout)
    assert torch.equal(out_h, out_f)
    assert torch.equal(bias_h.grad, bias_f.grad), "d/dbias"
    assert t.grad.dtype == dtype and t.grad.shape == t.shape
    _same16(t.grad, xf.grad.to(dtype), "d/dx rounded to the table's type")
    # float64 autograd on the widened table, test_gpu_backward.py's bars (2e-5 d/dx; 1e-4 for a bias gradient)
    x64 = t.detach().double().cpu().requires_grad_(True)
    b64 = bias_h.detach().double().cpu().requires_grad_(True)
    rows, cols = torch.from_numpy(ei[0]).long(), torch.from_numpy(ei[1]).long()
    agg = torch.zeros(n, F, dtype=torch.float64).index_add(0, rows, x64[cols] * w.double().cpu()[:, None]) + sc.double().cpu()[:, None] * x64
    if mean:
        agg = agg / torch.bincount(rows, minlength=n).clamp(min=1).double()[:, None]
    ref = torch.relu(agg + b64)
    ref.backward(gout.double().cpu())
    assert_parity(out_h.detach().cpu().numpy(), ref.detach().numpy(), what="forward")
    assert_parity(xf.grad.cpu().numpy(), x64.grad.numpy(), tol=2e-5, what="d/dx (float32, before rounding)")
    assert_parity(bias_h.grad.cpu().numpy(), b64.grad.numpy(), tol=1e-4, what="d/dbias")
    # a table built from a leaf by prepare_half_features carries no gradient; bias still trains
    leaf = torch.randn(n, F, device="cuda", requires_grad=True)
    hq = tfg.prepare_half_features(leaf, dtype=dtype)
    b2 = torch.zeros(F, device="cuda", requires_grad=True)
    AG.aggregate(plan, hq, op, w_csr, sc, bias=b2).sum().backward()
    assert leaf.grad is None and b2.grad is not None
    with pytest.raises(NotImplementedError):
        AG.aggregate(plan, hq, op, w_csr.clone().requires_grad_(True), sc)
    with pytest.raises(NotImplementedError):
        AG.aggregate(plan, P.HalfRows.from_tensor(t), L.MAX, w_csr)
    with torch.no_grad():
        assert torch.equal(AG.aggregate(plan, hq, L.MAX, w_csr), P.segment_reduce(plan, hq.float(), L.MAX, w_csr=w_csr))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_h16_gradient_reaches_the_source_through_every_term(tfg, dtype):
    """d/dt of HalfRows.from_tensor(t) through the public entries that ALSO read the widened table: the identity term of
    aggregate_neighbors(sum_updater) and the self half of MeanGraphSage.  Every term's float32 gradient is summed in float32
    and rounded once.  aggregate_neighbors: the float32 route computes the same float32 sum (g + A^T g), so the rounded
    gradient agrees bit for bit.  MeanGraphSage: the float32 layer runs the projection first (re-association), so the bar is
    half a unit in the last place of the 16-bit type (2^-8 bf16, 2^-11 fp16, relative) on top of twice test_gpu_backward.py's
    bar for a GraphSAGE layer's d/dx (5e-5 against float64 for EACH of the two float32 routes compared here)."""
    L = tfg._lib
    nnk = tfg.nn
    from tf_geometric_amd import plan as P
    rng = _rng(23500, 0)
    n, F, E = 150, 100, 2000
    ei = L.as_i32(rng.integers(0, n, size=(2, E)).astype(np.int32))
    w = L.as_f32(rng.uniform(0.2, 1.5, size=E).astype(np.float32))
    half_ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11      # 8 / 11 significand bits: ulp 2^-7 / 2^-10 of the binade
    torch.manual_seed(23500)

    def grads(fn, gout):
        t = t0.clone().requires_grad_(True)
        fn(P.HalfRows.from_tensor(t)).backward(gout)
        xf = t0.float().requires_grad_(True)
        fn(xf).backward(gout)
        assert t.grad is not None and t.grad.dtype == dtype and t.grad.shape == t.shape and t.grad.device == t.device
        return t.grad, xf.grad

    t0 = torch.randn(n, F, device="cuda").to(dtype)
    gout = torch.randn(n, F, device="cuda")
    for mapper, ew, reducer in ((nnk.gcn_mapper, w, nnk.sum_reducer), (nnk.identity_mapper, None, nnk.mean_reducer)):
        g16, g32 = grads(lambda x: nnk.aggregate_neighbors(x, ei, ew, mapper, reducer, nnk.sum_updater), gout)
        _same16(g16, g32.to(dtype), "aggregate_neighbors(sum_updater) d/dt, {}".format(reducer.__name__))
        # the identity term alone is gout: a gradient that misses it is off by gout
        g_id, _ = grads(lambda x: nnk.aggregate_neighbors(x, ei, ew, mapper, reducer, nnk.identity_updater), gout)
        assert not torch.equal(g16, g_id)
    layer = tfg.layers.MeanGraphSage(64)
    gl = torch.randn(n, 64, device="cuda")
    g16, g32 = grads(lambda x: layer([x, ei, w]), gl)
    err = (g16.float() - g32).abs() - (half_ulp + 1e-4) * g32.abs()
    assert float(err.max()) <= 1e-4, "MeanGraphSage d/dt: max(|d| - tol * |ref|) = {:.3e}".format(float(err.max()))
    # a gradient that misses the self half is off by gl[:, :32] @ self_kernel^T, of order 1: far outside that bar


# -------------------------------------------------------------------------------------------------------- 6. public surface
def test_h16_public_surface(tfg):
    L = tfg._lib
    nnk = tfg.nn
    rng = _rng(24000, 0)
    n, F, E = 300, 100, 6000
    ei = L.as_i32(rng.integers(0, n, size=(2, E)).astype(np.int32))
    w = L.as_f32(rng.uniform(0.2, 1.5, size=E).astype(np.float32))
    h = tfg.prepare_half_features(torch.randn(n, F, device="cuda"), dtype=torch.bfloat16)
    xf = h.float()
    for mapper, ew in ((nnk.identity_mapper, None), (nnk.gcn_mapper, w)):
        for reducer in (nnk.sum_reducer, nnk.mean_reducer, nnk.max_reducer):
            for updater in (nnk.sum_updater, nnk.identity_updater):
                a = nnk.aggregate_neighbors(h, ei, ew, mapper, reducer, updater)
                b = nnk.aggregate_neighbors(xf, ei, ew, mapper, reducer, updater)
                assert a.dtype == torch.float32 and torch.equal(a, b), (mapper.__name__, reducer.__name__, updater.__name__)
    with pytest.raises(TypeError):
        nnk.aggregate_neighbors(h, ei, w, lambda r, nx, edge_weight=None: nx * 2.0, nnk.sum_reducer, nnk.identity_updater)
    adj = tfg.SparseMatrix(ei, w, [n, n])
    assert torch.equal(adj @ h, adj @ xf)
    for cls in (tfg.layers.MeanGraphSage, tfg.layers.SumGraphSage):
        for units in (64, 256):
            layer = cls(units)
            with torch.no_grad():
                a = layer([h, ei, w])
                b = layer([xf, ei, w])
            assert a.shape == b.shape == (n, units)
            assert_parity(a.cpu().numpy(), b.cpu().numpy(), tol=1e-5, what="{}({})".format(cls.__name__, units))
    wide = tfg.prepare_half_features(torch.randn(n, 1433, device="cuda"))
    with pytest.raises(TypeError, match="before aggregating"):
        tfg.layers.GCN(16)([wide, ei])
    with pytest.raises(TypeError, match="before aggregating"):
        tfg.layers.GAT(16)([h, ei])


# ------------------------------------------------------------------------------------------------------------- 7. full size
def test_h16_products_shape(tfg):
    """products shape, F = 100, weighted, self_coef, bf16: the whole output equals the float32 route's (torch.equal), run to
    run bit-identical, 2000 sampled rows + the 10 longest against float64 on the widened table at 1e-5."""
    from tf_geometric_amd import synthetic
    from tf_geometric_amd import plan as P
    L = tfg._lib
    n, e, f = synthetic.WORKLOADS["products"]
    free, _ = torch.cuda.mem_get_info()
    if free < 16 << 30:
        pytest.skip("products-shaped 16-bit test needs 16 GB of free HBM, {:.1f} GB free".format(free / 2 ** 30))
    ei = L.as_i32(synthetic.synthetic_edges(n, e, seed=0))
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn(n, f, generator=g, device="cuda")
    w = torch.rand(int(ei.shape[1]), generator=g, device="cuda") + 0.5
    sc = torch.rand(n, generator=g, device="cuda") + 0.1
    plan = P.CsrPlan.build(ei, n, n)
    w_csr = plan.edge_attr_to_csr(w)
    h = tfg.prepare_half_features(x, dtype=torch.bfloat16)
    del x
    assert P.segment_reduce(plan, h, L.SUM, w_csr=w_csr, self_coef=sc, describe=True) == "seg_reduce_h16_kernel<1, 16, 1, false, true, 0>"
    got = P.segment_reduce(plan, h, L.SUM, w_csr=w_csr, self_coef=sc)
    again = P.segment_reduce(plan, h, L.SUM, w_csr=w_csr, self_coef=sc)
    assert torch.equal(got, again), "run to run"
    del again
    xf = h.float()
    with P.no_auto_promotion():
        exp = P.segment_reduce(plan, xf, L.SUM, w_csr=w_csr, self_coef=sc)
    assert torch.equal(got, exp), "16-bit route != float32 route at products shape"
    del exp
    gcpu = torch.Generator(device="cpu")
    gcpu.manual_seed(5)
    deg = plan.in_degree()
    rows = torch.unique(torch.cat([torch.randperm(n, generator=gcpu)[:2000].cuda(), torch.topk(deg, 10).indices.long()]))
    rp, col = plan.row_ptr.cpu().long(), plan.col.long()
    checked = 0
    for r in rows.tolist():
        s0, e0 = int(rp[r]), int(rp[r + 1])
        c = col[s0:e0]
        ref = (xf[c].double() * w_csr[s0:e0].double()[:, None]).sum(0) + sc[r].double() * xf[r].double()
        assert_parity(got[r].cpu().numpy(), ref.cpu().numpy().astype(np.float32), tol=1e-5,
                      what="products-shape bf16 row {}".format(r))
        checked += 1
    assert checked == int(rows.shape[0]) >= 2000
