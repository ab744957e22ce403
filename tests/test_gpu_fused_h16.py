# coding=utf-8
"""The fused aggregate -> project launch over a 16-bit table (include/tfgx_fused_h16.h) on the GPU.

Contract: tfgx_aggregate_gemm_h16 returns, BIT FOR BIT (torch.equal), what tfgx_aggregate_gemm_f32 returns for the table
widened to float32 with the same plan structures, for C and for the side output, run to run identical.  The independent
anchor — bit identity alone would pass a shared bug — is float64 numpy on the widened table at the bar of
test_gpu_fuzz.test_fuzz_fused_aggregate_gemm: 2e-5 * sqrt(max column sum of |messages|) for the aggregate, times
max(1, max column sum of |B|) for C.  Draws: test_fused_h16_abi.draw_fused_h16 (its census asserts without a device that the
default seeds reach every instantiation, resident and streamed B, hub and non-hub plans)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_parity
from test_fused_h16_abi import BF16, N_FH, _SCALE, _target_of, draw_fused_h16, fused_h16_kernel_name
from test_gpu_fuzz_backward import _rng
from test_gpu_h16 import _fill16, _nan32, _same16, _still_nan32

pytestmark = pytest.mark.gpu
_TORCH_DT = {BF16: torch.bfloat16, 2: torch.float16}


def _desc(d):
    return " ".join("{}={}".format(k, d[k]) for k in ("seed", "setting", "n_dst", "n_src", "F", "N", "dt", "weighted", "ldx", "mean",
                                                      "self", "bias", "relu", "side", "count_extra", "hub"))


@pytest.mark.parametrize("seed", range(N_FH * _SCALE))
def test_fused_h16_bit_identity_and_float64(tfg, seed):
    from tf_geometric_amd import plan as P
    L = tfg._lib
    lib = L.require_gpu()
    d = draw_fused_h16(seed)
    what = "fused h16 " + _desc(d)
    rng = _rng(31500, seed)
    F, N, n_src, n_dst, ei, ldx = d["F"], d["N"], d["n_src"], d["n_dst"], d["ei"], d["ldx"]
    dtype = _TORCH_DT[d["dt"]]
    E = ei.shape[1]
    x32 = rng.standard_normal((n_src, F)).astype(np.float32)
    k = (rng.standard_normal((F, N)) / np.sqrt(F)).astype(np.float32)
    w = rng.uniform(-1.5, 1.5, size=E).astype(np.float32) if d["weighted"] else None
    sc = rng.uniform(0.1, 1.0, size=n_dst).astype(np.float32) if d["self"] else None
    bias = rng.standard_normal(N).astype(np.float32) if d["bias"] else None
    deg = np.bincount(ei[0], minlength=n_dst)
    count = deg + (rng.integers(1, 4, size=n_dst) if d["count_extra"] else 0)      # a mean_count that is not the row length
    old = P.HUB_THRESHOLD, P.HUB_CHUNK
    try:
        if d["hub"]:
            P.HUB_THRESHOLD, P.HUB_CHUNK = d["hub"]
        plan = P.CsrPlan.build(L.as_i32(ei), n_dst, n_src)
        hub = plan.hub_info()
        assert (hub is not None) or not d["setting"].startswith("hub"), what
        # the 16-bit table: torch's rounding on the host, pad columns hold a NaN bit pattern
        table = _fill16((n_src, ldx), dtype)
        table[:, :F] = torch.from_numpy(x32).to(dtype).cuda()
        H = P.HalfRows(table, F)
        xf = H.float()
        assert torch.equal(xf, table[:, :F].float())
        kd = L.as_f32(k)
        bd = None if bias is None else L.as_f32(bias)
        wd = None if w is None else plan.edge_attr_to_csr(w)
        scd = None if sc is None else L.as_f32(sc)
        cnt = L.as_i32(count) if d["count_extra"] else None
        order = slot = None
        if d["row_order"]:      # rows by descending length (a permutation: results must not depend on it)
            order = torch.argsort(plan.in_degree(), descending=True, stable=True).to(torch.int32)
            if d["slot"] and hub is not None:
                slot = torch.searchsorted(hub[0], order[:int(hub[0].shape[0])].contiguous()).to(torch.int32)
        keep = []

        def launch(half):
            """One call at the C ABI on fresh NaN-filled buffers -> (wide C, C block, wide side, side block)."""
            a = L.ReduceArgs()
            a.row_begin, a.row_end, a.rp_stride = plan.row_ptr.data_ptr(), plan.row_ptr[1:].data_ptr(), 1
            a.col = plan.col.data_ptr()
            a.w = 0 if wd is None else wd.data_ptr()
            a.n_dst, a.F, a.op = n_dst, F, L.MEAN if d["mean"] else L.SUM
            a.x, a.ldx = (table.data_ptr(), ldx) if half else (xf.data_ptr(), F)
            a.self_coef = 0 if scd is None else scd.data_ptr()
            a.mean_count = 0 if cnt is None else cnt.data_ptr()
            if order is not None:
                a.row_order = order.data_ptr()
            if hub is not None:
                scratch = _nan32((int(hub[2].shape[0]), F))
                keep.append(scratch)
                a.hub_threshold = plan.hub_threshold
                a.hub_rows, a.hub_chunk_ptr, a.hub_chunk_begin, a.hub_chunk_end = (t.data_ptr() for t in hub[:4])
                a.n_hub_rows, a.n_hub_chunks, a.hub_scratch = int(hub[0].shape[0]), int(hub[2].shape[0]), scratch.data_ptr()
                if slot is not None:
                    a.hub_order_slot = slot.data_ptr()
            wide_c = _nan32((n_dst, d["c_off"] + N + d["c_pad"]))
            c = wide_c[:, d["c_off"]:d["c_off"] + N]
            wide_s = side = None
            if d["side"]:
                wide_s = _nan32((n_dst, d["s_off"] + F + d["s_pad"]))
                side = wide_s[:, d["s_off"]:d["s_off"] + F]
                a.out, a.ldo = side.data_ptr(), int(wide_s.shape[1])
            act = L.ACT_RELU if d["relu"] else L.ACT_NONE
            if half:
                buf = ctypes.create_string_buffer(160)
                L.check(lib.tfgx_aggregate_gemm_h16_describe(ctypes.byref(a), d["dt"], N, buf, 160), "describe")
                assert buf.value.decode() == fused_h16_kernel_name(d["dt"], F, w is not None) and _target_of(buf.value.decode()) == d["target"]
                L.check(lib.tfgx_aggregate_gemm_h16(ctypes.byref(a), d["dt"], L.ptr(kd), N, L.ptr(bd), act, c.data_ptr(),
                                                    int(wide_c.shape[1]), N, L.stream_ptr()), "tfgx_aggregate_gemm_h16")
            else:
                L.check(lib.tfgx_aggregate_gemm_f32(ctypes.byref(a), L.ptr(kd), N, L.ptr(bd), act, c.data_ptr(), int(wide_c.shape[1]), N,
                                                    L.stream_ptr()), "tfgx_aggregate_gemm_f32")
            return wide_c, c, wide_s, side

        wide_c, got, wide_s, side = launch(True)
        _, again, _, side_again = launch(True)
        _, exp, _, side_exp = launch(False)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(got).any()), what + ": NaN reached C (pad columns?)"
        assert torch.equal(got, again), what + ": run to run"
        assert torch.equal(got, exp), "{}: C differs from the float32 launch on the widened table ({} elements)".format(
            what, int((got.contiguous().view(torch.int32) != exp.contiguous().view(torch.int32)).sum()))
        assert _still_nan32(wide_c[:, :d["c_off"]]) and _still_nan32(wide_c[:, d["c_off"] + N:]), what + ": columns outside C's block"
        if d["side"]:
            assert not bool(torch.isnan(side).any()), what + ": NaN reached the side output"
            assert torch.equal(side, side_again) and torch.equal(side, side_exp), what + ": side output"
            assert _still_nan32(wide_s[:, :d["s_off"]]) and _still_nan32(wide_s[:, d["s_off"] + F:]), what + ": columns outside the side block"
        # float64 restatement on the widened table
        x = xf.cpu().numpy()
        msg = x[ei[1]].astype(np.float64) * (w[:, None] if w is not None else 1.0)
        agg = np.zeros((n_dst, F))
        np.add.at(agg, ei[0], msg)
        if sc is not None:
            agg += sc[:, None].astype(np.float64) * x[:n_dst]
        if d["mean"]:
            agg /= np.maximum(count, 1)[:, None]
        ref = agg @ k.astype(np.float64)
        if bias is not None:
            ref = ref + bias
        if d["relu"]:
            ref = np.maximum(ref, 0)
        scale = max(1.0, float(np.abs(msg).sum(0).max()) if E else 1.0)
        tol = 2e-5 * scale ** 0.5
        if d["side"]:
            assert_parity(side.cpu().numpy(), agg.astype(np.float32), tol=tol, what=what + " (side output vs float64)")
        assert_parity(got.cpu().numpy(), ref.astype(np.float32), tol=tol * max(1.0, float(np.abs(k).sum(0).max())), what=what + " vs float64")
    finally:
        P.HUB_THRESHOLD, P.HUB_CHUNK = old


def _layer_graph(seed, n=300, F=100, E=6000):
    rng = _rng(32000, seed)
    ei = torch.from_numpy(rng.integers(0, n, size=(2, E)).astype(np.int32)).cuda()
    w = torch.from_numpy(rng.uniform(0.2, 1.5, size=E).astype(np.float32)).cuda()
    return rng, ei, w


def test_fused_h16_layers_inference(tfg):
    """GCN(256) (and kernel=None) and Mean / SumGraphSage(256) on a bf16 HalfRows, F = 100: torch.equal to the layer on
    h.float() — both take their fused launch (FUSED_STATS) — one launch per call; the GEMM-first GCN and GAT still refuse."""
    from tf_geometric_amd import plan as P
    n, F = 300, 100
    _, ei, w = _layer_graph(0, n, F)
    h = tfg.prepare_half_features(torch.randn(n, F, device="cuda"), dtype=torch.bfloat16)
    xf = h.float()
    for make in (lambda: tfg.layers.GCN(256, activation=tfg.relu), lambda: tfg.layers.MeanGraphSage(256, activation=tfg.relu),
                 lambda: tfg.layers.SumGraphSage(256)):
        layer = make()
        with torch.no_grad():
            b0, h0 = P.FUSED_STATS["launches"], P.FUSED_H16_STATS["launches"]
            a = layer([h, ei, w])
            assert P.FUSED_STATS["launches"] == b0 + 1 and P.FUSED_H16_STATS["launches"] == h0 + 1, type(layer).__name__
            b = layer([xf, ei, w], cache={})
            both_fused = P.FUSED_STATS["launches"] == b0 + 2 and P.FUSED_H16_STATS["launches"] == h0 + 1
        assert a.shape == b.shape == (n, 256) and a.dtype == torch.float32
        assert both_fused, "the float32 layer left its fused launch at this shape"
        assert torch.equal(a, b), type(layer).__name__
    # kernel=None: the aggregation alone, tfgx_segment_reduce_h16 — the float32 route's bits
    adj = tfg.SparseMatrix(ei, w, [n, n])
    with torch.no_grad():
        a = tfg.nn.gcn(h, adj, None, bias=torch.ones(F, device="cuda"), activation=tfg.relu)
        b = tfg.nn.gcn(xf, adj, None, bias=torch.ones(F, device="cuda"), activation=tfg.relu)
    assert_parity(a.cpu().numpy(), b.cpu().numpy(), tol=1e-5, what="gcn(kernel=None)")
    assert torch.equal(a, b)
    # a width the fused launch does not take (F = 132): segment_reduce on the 16-bit table + float32 GEMM, inside 1e-5
    h2 = tfg.prepare_half_features(torch.randn(n, 132, device="cuda"), dtype=torch.float16)
    layer = tfg.layers.GCN(256)
    with torch.no_grad():
        b0 = P.FUSED_H16_STATS["launches"]
        a, b = layer([h2, ei, w]), layer([h2.float(), ei, w], cache={})
        assert P.FUSED_H16_STATS["launches"] == b0
    assert_parity(a.cpu().numpy(), b.cpu().numpy(), tol=1e-5, what="GCN(256) on F = 132 (two launches)")
    wide = tfg.prepare_half_features(torch.randn(n, 1433, device="cuda"))
    with pytest.raises(TypeError, match="before aggregating"):
        tfg.layers.GCN(16)([wide, ei])
    with pytest.raises(TypeError, match="before aggregating"):
        tfg.layers.GCN(100)([h, ei])
    with pytest.raises(TypeError, match="before aggregating"):
        tfg.layers.GAT(16)([h, ei])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", ["gcn", "mean_sage"])
def test_fused_h16_layers_training(tfg, oracle, kind, dtype):
    """GCN(256) / MeanGraphSage(256) on HalfRows.from_tensor(t), t.requires_grad: kernel / bias gradients against float64
    autograd of the dense restatement on t.float() (tests/f64_layers.py) at test_gpu_backward.py's bars for the float32 fused
    training route (2e-4; forward 1e-5); d/dt, rounded to the table's type, within half a 16-bit ulp (2^-8 bf16, 2^-11 fp16,
    relative) plus that file's d/dx bar (5e-5), as test_gpu_h16.py states it.  One fused launch with its side output."""
    import f64_layers as R
    from tf_geometric_amd import plan as P
    n, F, units = 300, 100, 256
    rng, ei, w = _layer_graph(1, n, F)
    half_ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    torch.manual_seed(32001)
    t = torch.randn(n, F, device="cuda").to(dtype).requires_grad_(True)
    G = torch.randn(n, units, device="cuda")
    if kind == "gcn":
        layer = tfg.layers.GCN(units, activation=tfg.relu)
        ws = {"kernel": oracle.glorot_uniform(rng, F, units), "bias": (rng.standard_normal(units) * 0.1).astype(np.float32)}
        ref_out, ref, G_eff = R.gcn_layer(t.detach().float(), ei, w, ws["kernel"], ws["bias"], G)
    else:
        layer = tfg.layers.MeanGraphSage(units, activation=tfg.relu, concat=True)
        ku = units // 2
        ws = {"self_kernel": oracle.glorot_uniform(rng, F, ku), "neighbor_kernel": oracle.glorot_uniform(rng, F, ku),
              "bias": (rng.standard_normal(units) * 0.3).astype(np.float32)}
        ref_out, ref, G_eff = R.mean_sage_layer(t.detach().float(), ei, w, ws["self_kernel"], ws["neighbor_kernel"], ws["bias"], G)
    layer._maybe_build([t.detach().float()])
    layer.set_weights(**ws)
    layer.trainable(True)
    before, before_h = dict(P.FUSED_STATS), P.FUSED_H16_STATS["launches"]
    out = layer([P.HalfRows.from_tensor(t), ei, w], cache={})
    assert P.FUSED_STATS["launches"] == before["launches"] + 1 and P.FUSED_H16_STATS["launches"] == before_h + 1
    assert P.FUSED_STATS["with_side_output"] == before["with_side_output"] + 1      # the kernel's gradient needs the aggregate
    out.backward(G_eff.to(out.device))
    assert_parity(out.detach().cpu().numpy(), ref_out.cpu().numpy(), what=kind + " forward")
    for k_ in ws:
        assert_parity(getattr(layer, k_).grad.cpu().numpy(), ref[k_].cpu().numpy(), tol=2e-4, what=kind + " d/d" + k_)
    assert t.grad is not None and t.grad.dtype == dtype and t.grad.shape == t.shape
    r64 = ref["x"].cpu().double()
    err = (t.grad.cpu().double() - r64).abs() - (half_ulp + 5e-5) * r64.abs()
    assert float(err.max()) <= 5e-5, "{} d/dt: max(|d| - tol * |ref|) = {:.3e}".format(kind, float(err.max()))
    # the float32 fused training route on t.float(): same forward bits, d/dt = its d/dx rounded once
    for p_ in layer.parameters() if hasattr(layer, "parameters") else []:
        p_.grad = None
    xf = t.detach().float().requires_grad_(True)
    out_f = layer([xf, ei, w], cache={})
    assert torch.equal(out_f, out), kind + ": forward differs from the float32 fused route"
    out_f.backward(G_eff.to(out.device))
    _same16(t.grad, xf.grad.to(dtype), kind + " d/dt vs the float32 route's d/dx rounded")
    # a table quantised from a leaf carries no gradient; the kernel still trains
    leaf = torch.randn(n, F, device="cuda", requires_grad=True)
    hq = tfg.prepare_half_features(leaf, dtype=dtype)
    layer([hq, ei, w], cache={}).sum().backward()
    assert leaf.grad is None
    if kind == "gcn":
        from tf_geometric_amd import autograd as AG
        plan = P.CsrPlan.build(ei, n, n)
        with pytest.raises(NotImplementedError):
            AG.aggregate_project(plan, hq, tfg._lib.SUM, layer.kernel, plan.edge_attr_to_csr(w).clone().requires_grad_(True))


# --------------------------------------------------------------------------------- the 16-bit and float32 routes, case by case
_TWIN_ENTRIES = ("aggregate", "aggregate_project", "sage_wide")
_TWIN_N, _TWIN_F, _TWIN_UNITS, _TWIN_E = 70, 100, 256, 800      # one full 64-row tile plus a remainder


def twin_cases(entry):
    """bias x ReLU x kernel(s) trainable x table's source trainable x mean x (aggregate, aggregate_project) trainable self_coef;
    `aggregate` has no kernel, and takes one rectangular case more (n_dst = 1 < n_src with a self_coef)."""
    import itertools
    for bias, relu, k_grad, t_grad, mean, self_ in itertools.product((False, True), repeat=6):
        if (entry == "aggregate" and k_grad) or (entry == "sage_wide" and self_):
            continue
        yield dict(bias=bias, relu=relu, k_grad=k_grad, t_grad=t_grad, mean=mean, self=self_, n_dst=_TWIN_N)
    if entry == "aggregate":
        yield dict(bias=True, relu=True, k_grad=False, t_grad=True, mean=True, self=True, n_dst=1)


def twin_graph(tfg, n_dst):
    """(plan [n_dst x _TWIN_N], constant edge weights in CSR order)."""
    from tf_geometric_amd import plan as P
    rng = _rng(32100, n_dst)
    E = _TWIN_E if n_dst > 1 else 23
    ei = np.stack([rng.integers(0, n_dst, size=E), rng.integers(0, _TWIN_N, size=E)]).astype(np.int32)
    plan = P.CsrPlan.build(tfg._lib.as_i32(ei), n_dst, _TWIN_N)
    return plan, plan.edge_attr_to_csr(rng.uniform(0.2, 1.5, size=E).astype(np.float32))


def twin_run(tfg, entry, c, plan, w_csr, t, G, half):
    """One public entry point of autograd.py on HalfRows.from_tensor(t) (half) or on t.float(), same weights, same upstream
    gradient -> (forward, {name: gradient}, (fused launches, with side output, fused launches over a 16-bit table))."""
    from tf_geometric_amd import plan as P, autograd as AG
    L = tfg._lib
    rng = _rng(32101, 0)

    def leaf(a, grad):
        return torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda().requires_grad_(grad)
    F = int(t.shape[1])
    src = (t.detach().clone() if half else t.detach().float()).requires_grad_(c["t_grad"])
    x = P.HalfRows.from_tensor(src) if half else src
    op, act = (L.MEAN if c["mean"] else L.SUM), (L.ACT_RELU if c["relu"] else L.ACT_NONE)
    ku = _TWIN_UNITS // 2
    leaves = {"source": src}
    if entry == "aggregate_project":
        leaves["kernel"] = leaf(rng.standard_normal((F, _TWIN_UNITS)) / F ** 0.5, c["k_grad"])
    elif entry == "sage_wide":
        leaves["self_kernel"] = leaf(rng.standard_normal((F, ku)) / F ** 0.5, c["k_grad"])
        leaves["neighbor_kernel"] = leaf(rng.standard_normal((F, ku)) / F ** 0.5, c["k_grad"])
    if c["bias"]:
        leaves["bias"] = leaf(rng.standard_normal(F if entry == "aggregate" else _TWIN_UNITS) * 0.3, True)
    if c["self"]:
        leaves["self_coef"] = leaf(rng.uniform(0.1, 1.0, size=plan.n_dst), True)
    bias, sc = leaves.get("bias"), leaves.get("self_coef")
    before = (P.FUSED_STATS["launches"], P.FUSED_STATS["with_side_output"], P.FUSED_H16_STATS["launches"])
    if entry == "aggregate":
        out = AG.aggregate(plan, x, op, w_csr, sc, bias=bias, act=act)
    elif entry == "aggregate_project":
        assert P.aggregate_gemm_applies(x, leaves["kernel"], op)
        out = AG.aggregate_project(plan, x, op, leaves["kernel"], w_csr, sc, bias, act)
    else:
        assert P.aggregate_gemm_applies(x, leaves["neighbor_kernel"], op)
        out = AG.sage_wide(plan, op, x, leaves["self_kernel"], leaves["neighbor_kernel"], w_csr, bias, act)
    stats = (P.FUSED_STATS["launches"] - before[0], P.FUSED_STATS["with_side_output"] - before[1],
             P.FUSED_H16_STATS["launches"] - before[2])
    assert out is not None and out.requires_grad == any(v.requires_grad for v in leaves.values())
    if out.requires_grad:
        out.backward(G)
    return out.detach(), {k: v.grad for k, v in leaves.items() if v.requires_grad}, stats


def twin_inputs(tfg, entry, dtype):
    """(16-bit table values [n, F], {n_dst: (plan, w_csr, upstream gradient)}) of one (entry point, dtype)."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(32102)
    t = torch.randn(_TWIN_N, _TWIN_F, generator=gen, device="cuda").to(dtype)
    graphs = {}
    for n_dst in sorted({c["n_dst"] for c in twin_cases(entry)}):
        G = torch.randn(n_dst, _TWIN_F if entry == "aggregate" else _TWIN_UNITS, generator=gen, device="cuda")
        graphs[n_dst] = twin_graph(tfg, n_dst) + (G,)
    return t, graphs


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("entry", _TWIN_ENTRIES)
def test_fused_h16_route_equals_float32_route(tfg, entry, dtype):
    """autograd.aggregate / aggregate_project / sage_wide on HalfRows.from_tensor(t) against the same call on t.float(), over
    every combination of twin_cases: the forward and every float32 gradient (kernels, bias, self_coef) torch.equal, d/dt the
    float32 route's d/dx rounded once to t.dtype (bit for bit), one fused launch per call on either route (none for aggregate)
    with the aggregate written beside it exactly when the kernel's gradient is wanted."""
    t, graphs = twin_inputs(tfg, entry, dtype)
    for c in twin_cases(entry):
        what = "{} {} {}".format(entry, dtype, " ".join("{}={}".format(k, int(v)) for k, v in c.items()))
        plan, w_csr, G = graphs[c["n_dst"]]
        out_h, grads_h, stats_h = twin_run(tfg, entry, c, plan, w_csr, t, G, True)
        out_f, grads_f, stats_f = twin_run(tfg, entry, c, plan, w_csr, t, G, False)
        fused = int(entry != "aggregate")
        assert stats_h == (fused, int(fused and c["k_grad"]), fused), what + ": launches over the 16-bit table"
        assert stats_f == (fused, int(fused and c["k_grad"]), 0), what + ": launches over the float32 table"
        assert out_h.dtype == torch.float32 and torch.equal(out_h, out_f), what + ": forward"
        assert sorted(grads_h) == sorted(grads_f), what
        for k in grads_f:
            assert grads_h[k] is not None and grads_f[k] is not None, what + ": no d/d" + k
            if k == "source":
                assert grads_h[k].dtype == dtype and grads_h[k].shape == t.shape, what
                _same16(grads_h[k], grads_f[k].to(dtype), what + " d/dt vs the float32 route's d/dx rounded")
            else:
                assert torch.equal(grads_h[k], grads_f[k]), what + ": d/d" + k
