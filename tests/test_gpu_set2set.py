# coding=utf-8
"""Set2Set on the GPU (tfgx_set2set.h, layers.LSTM.call, nn.set2set, layers.Set2Set) against the float64 mirror of
tests/set2set_mirror.py, which tests/test_set2set_abi.py pins to the reference's own outputs.

Tolerance (per case and per tensor), the rule of tests/test_gpu_lstm_sage.py: the same mirror evaluated in float32 on the CPU
is an independent f32 evaluation of the case; the GPU result may differ from the float64 mirror by 4x that f32-CPU error,
with a floor of 1e-6 absolute.  Every figure is printed before it is asserted.

Shapes: graph sizes 0 / 1 / C-1 / C / C+1 / 2C+1 (C = TFGX_SET2SET_CHUNK_ROWS) in one batch put an uncut graph, a graph of
exactly one chunk and graphs of two and three chunks side by side; F 1 .. 256 crosses the one-lane, part-wave, full-wave and
several-columns-per-lane row shapes in both the 4-byte (F = 1, 3, 65) and the 16-byte form; U = 96 / 112 straddle
tfgx_lstm_sequence_kernel_resident."""
import os
import sys

import numpy as np
import pytest
import torch

import set2set_mirror as M
from conftest import ROOT
from set2set_mirror import golden_cases, mirror_of_case
from tf_geometric_amd._lib import SET2SET_CHUNK_ROWS as CHUNK

pytestmark = pytest.mark.gpu


def check(what, gpu, ref, cpu32):
    cpu_err = float((cpu32.double() - ref).abs().max()) if ref.numel() else 0.0
    gpu_err = float((gpu.double() - ref).abs().max()) if ref.numel() else 0.0
    tol = max(4.0 * cpu_err, 1e-6)
    print("{}: cpu-f32 err {:.3e}  gpu err {:.3e}  tol {:.3e}".format(what, cpu_err, gpu_err, tol))
    assert tuple(gpu.shape) == tuple(ref.shape), what
    assert bool(torch.isfinite(gpu).all()), "{}: non-finite".format(what)
    assert gpu_err <= tol, "{}: gpu err {:.3e} > tol {:.3e} (cpu-f32 err {:.3e})".format(what, gpu_err, tol, cpu_err)


# ---- the attention kernels through the C ABI ----------------------------------------------------------------------------------
SIZES = [0, 1, CHUNK - 1, 0, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 0]      # empty graphs first, in the middle and last


def graph_ids(shuffled, seed=0):
    ids = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
    if shuffled:
        ids = ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(seed))]
    return ids


def csr_of(ids, G):
    order = torch.sort(ids, stable=True).indices
    row_ptr = torch.zeros(G + 1, dtype=torch.long)
    row_ptr[1:] = torch.cumsum(torch.bincount(ids, minlength=G), 0)
    return row_ptr.to(torch.int32), order.to(torch.int32)


def attend_reference(x, ids, q, G, gout, dtype):
    xx, qq = x.detach().clone().to(dtype).requires_grad_(True), q.detach().clone().to(dtype).requires_grad_(True)
    r, _ = M.attend_mirror(xx, ids, qq, G)
    (r * gout.to(dtype)).sum().backward()
    return r.detach().double(), xx.grad.double(), qq.grad.double()


def attend_gpu(tfg, row_ptr, node, x, q, G, gout, pad=0, want_flag=False, d_x_fill=None):
    """Forward and backward through the raw C ABI; `pad` extra columns make every leading dimension larger than F."""
    L = tfg._lib
    lib, dev = L.require_gpu(), L.device()
    N, F = x.shape
    ld = F + pad

    def padded(t):
        buf = torch.full((t.shape[0], ld), 7.0, dtype=torch.float32)
        buf[:, :F] = t.float()
        return buf.to(dev)

    xd, qd, gd = padded(x), padded(q), padded(gout)
    rp, nd = row_ptr.to(dev), node.to(dev)
    r = torch.full((G, ld), 7.0, dtype=torch.float32, device=dev)
    stats = torch.empty((G, 2), dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ws_bytes = lib.tfgx_set2set_attend_workspace_bytes(N, G, F)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    L.check(lib.tfgx_set2set_attend_f32(L.ptr(rp), L.ptr(nd), G, N, L.ptr(xd), ld, F, L.ptr(qd), ld, L.ptr(r), ld, L.ptr(stats),
                                        L.ptr(ws), ws_bytes, L.ptr(flag), L.stream_ptr()), "tfgx_set2set_attend_f32")
    r_inf = torch.full((G, ld), 7.0, dtype=torch.float32, device=dev)          # the inference call: no statistics
    L.check(lib.tfgx_set2set_attend_f32(L.ptr(rp), L.ptr(nd), G, N, L.ptr(xd), ld, F, L.ptr(qd), ld, L.ptr(r_inf), ld, None,
                                        L.ptr(ws), ws_bytes, None, L.stream_ptr()), "tfgx_set2set_attend_f32")
    assert torch.equal(r, r_inf), "the inference call differs from the training call"
    d_x = torch.full((N, ld), 7.0 if d_x_fill is None else d_x_fill, dtype=torch.float32, device=dev)
    d_q = torch.full((G, ld), 7.0, dtype=torch.float32, device=dev)
    L.check(lib.tfgx_set2set_attend_backward_f32(L.ptr(rp), L.ptr(nd), G, N, L.ptr(xd), ld, F, L.ptr(qd), ld, L.ptr(r), ld,
                                                 L.ptr(stats), L.ptr(gd), ld, L.ptr(d_x), ld, L.ptr(d_q), ld, L.ptr(ws), ws_bytes,
                                                 L.stream_ptr()), "tfgx_set2set_attend_backward_f32")
    for name, t in (("r", r), ("d_x", d_x), ("d_q", d_q)):
        if pad:
            assert bool((t[:, F:] == 7.0).all()), "{}: the kernel wrote past F".format(name)
    out = r[:, :F].cpu(), d_x[:, :F].cpu(), d_q[:, :F].cpu()
    return out + (int(flag.item()),) if want_flag else out


def attend_case(F, shuffled, scale=1.0, seed=1):
    g = torch.Generator().manual_seed(seed + F)
    ids = graph_ids(shuffled, seed)
    G, N = len(SIZES), ids.numel()
    x = torch.randn(N, F, generator=g, dtype=torch.float64) * scale
    q = torch.randn(G, F, generator=g, dtype=torch.float64) * scale
    gout = torch.randn(G, F, generator=g, dtype=torch.float64)
    return ids, x, q, gout, G


REF_CACHE = {}


def attend_refs(key, ids, x, q, G, gout):
    if key not in REF_CACHE:
        REF_CACHE[key] = (attend_reference(x, ids, q, G, gout, torch.float64), attend_reference(x, ids, q, G, gout, torch.float32))
    return REF_CACHE[key]


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("F", [1, 3, 16, 64, 65, 100, 256])
def test_attend_kernels_against_float64(tfg, F, shuffled):
    ids, x, q, gout, G = attend_case(F, shuffled)
    ref, cpu = attend_refs((F, shuffled), ids, x, q, G, gout)
    row_ptr, node = csr_of(ids, G)
    got = attend_gpu(tfg, row_ptr, node, x, q, G, gout)
    for name, a, b, c in zip(("r", "d_x", "d_q"), got, ref, cpu):
        check("attend F={} {} {}".format(F, "shuffled" if shuffled else "sorted", name), a, b, c)
    again = attend_gpu(tfg, row_ptr, node, x, q, G, gout)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two runs differ"


@pytest.mark.parametrize("F, pad", [(16, 4), (16, 3), (65, 2), (256, 8)])
def test_attend_with_a_leading_dimension_above_F(tfg, F, pad):
    """pad 4 / 8 keep the 16-byte row form at a stride above F, pad 3 / 2 force the 4-byte form."""
    ids, x, q, gout, G = attend_case(F, True)
    ref, cpu = attend_refs((F, True), ids, x, q, G, gout)
    row_ptr, node = csr_of(ids, G)
    got = attend_gpu(tfg, row_ptr, node, x, q, G, gout, pad=pad)
    for name, a, b, c in zip(("r", "d_x", "d_q"), got, ref, cpu):
        check("attend F={} pad={} {}".format(F, pad, name), a, b, c)


def test_attend_scores_of_magnitude_100(tfg):
    """|e| ~ 100: exp(e) overflows float32 without the running maximum."""
    F = 16
    ids, x, q, gout, G = attend_case(F, True, scale=5.0, seed=3)
    e = (x * q[ids]).sum(-1)
    assert float(e.abs().max()) > 100.0 and not bool(torch.isfinite(torch.exp(e.float())).all())
    ref = attend_reference(x, ids, q, G, gout, torch.float64)
    cpu = attend_reference(x, ids, q, G, gout, torch.float32)
    row_ptr, node = csr_of(ids, G)
    got = attend_gpu(tfg, row_ptr, node, x, q, G, gout)
    for name, a, b, c in zip(("r", "d_x", "d_q"), got, ref, cpu):
        check("attend big scores {}".format(name), a, b, c)


def test_attend_skips_an_out_of_range_node(tfg):
    """A valid buffer holding out-of-range VALUES: those entries are skipped, the flag is raised, and the d_x rows that the
    list no longer names keep what the caller put there.  The clean call leaves the flag at 0."""
    F = 16
    ids, x, q, gout, G = attend_case(F, True, seed=4)
    row_ptr, node = csr_of(ids, G)
    N = ids.numel()
    *_, flag = attend_gpu(tfg, row_ptr, node, x, q, G, gout, want_flag=True)
    assert flag == 0
    bad = node.clone()
    dropped = [int(row_ptr[2]) + 5, int(row_ptr[6]) + CHUNK + 3, int(row_ptr[7]) - 1]
    lost = bad[dropped].long()
    bad[dropped[0]], bad[dropped[1]], bad[dropped[2]] = N, -1, 2 ** 31 - 1
    keep = torch.ones(N, dtype=torch.bool)
    keep[lost] = False
    ref = attend_reference(x[keep], ids[keep], q, G, gout, torch.float64)
    cpu = attend_reference(x[keep], ids[keep], q, G, gout, torch.float32)
    r, d_x, d_q, flag = attend_gpu(tfg, row_ptr, bad, x, q, G, gout, want_flag=True, d_x_fill=-3.0)
    assert flag == 1
    assert bool((d_x[lost] == -3.0).all()), "a d_x row that the list does not name was written"
    check("bad node r", r, ref[0], cpu[0])
    check("bad node d_x", d_x[keep], ref[1], cpu[1])
    check("bad node d_q", d_q, ref[2], cpu[2])


# ---- the sequence LSTM through the C ABI --------------------------------------------------------------------------------------
def sequence_reference(P, R, h0, c0, B, T, U, gouts, dtype):
    eye = torch.eye(4 * U, dtype=dtype)
    t = [v.detach().clone().to(dtype).requires_grad_(True) for v in (P, R, h0, c0)]
    seq, h, c = M.lstm_mirror(t[0].reshape(B, T, 4 * U), eye, t[1], torch.zeros(4 * U, dtype=dtype), t[2], t[3])
    outs = (seq.reshape(B * T, U), h, c)
    loss = sum((o * g.to(dtype)).sum() for o, g in zip(outs, gouts) if g is not None)
    loss.backward()
    return [o.detach().double() for o in outs], [v.grad.double() for v in t]


def sequence_gpu(tfg, P, R, h0, c0, B, T, U, masks, gouts, zero_state):
    L = tfg._lib
    lib, dev = L.require_gpu(), L.device()
    d = lambda v: None if v is None else v.float().contiguous().to(dev)      # noqa: E731
    Pd, Rd = d(P), d(R)
    h0d, c0d = (None, None) if zero_state else (d(h0), d(c0))
    e = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)      # noqa: E731
    h_seq, h_last, c_last = e(B * T, U), e(B, U), e(B, U)
    saved = torch.empty(lib.tfgx_lstm_sequence_saved_bytes(B, T, U), dtype=torch.uint8, device=dev)
    L.check(lib.tfgx_lstm_sequence_f32(L.ptr(Pd), 4 * U, B, T, L.ptr(Rd), U, L.ptr(h0d), L.ptr(c0d), L.ptr(h_seq), L.ptr(h_last),
                                       L.ptr(c_last), L.ptr(saved), saved.numel(), L.stream_ptr()), "tfgx_lstm_sequence_f32")
    inf = e(B * T, U)
    L.check(lib.tfgx_lstm_sequence_f32(L.ptr(Pd), 4 * U, B, T, L.ptr(Rd), U, L.ptr(h0d), L.ptr(c0d), L.ptr(inf), None, None, None,
                                       0, L.stream_ptr()), "tfgx_lstm_sequence_f32")
    assert torch.equal(inf, h_seq), "the inference call differs from the training call"
    grads = []
    for mask in masks:
        gs = [d(g) if m else None for g, m in zip(gouts, mask)]
        d_gates, h_prev, d_h0, d_c0 = e(B * T, 4 * U), e(B * T, U), e(B, U), e(B, U)
        L.check(lib.tfgx_lstm_sequence_backward_f32(B, T, U, L.ptr(Rd), L.ptr(h0d), L.ptr(gs[0]), L.ptr(gs[1]), L.ptr(gs[2]),
                                                    L.ptr(saved), saved.numel(), L.ptr(d_gates), L.ptr(h_prev), L.ptr(d_h0),
                                                    L.ptr(d_c0), L.stream_ptr()), "tfgx_lstm_sequence_backward_f32")
        dR = tfg.plan.gemm_tn(h_prev, d_gates)[0]
        grads.append([v.cpu() for v in (d_gates, dR, d_h0, d_c0)])
    return [v.cpu() for v in (h_seq, h_last, c_last)], grads


MASKS = [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)]      # which of d_h_seq, d_h_last, d_c_last is given


@pytest.mark.parametrize("zero_state", [True, False], ids=["zero_state", "state"])
@pytest.mark.parametrize("B, T, U", [(1, 1, 16), (1, 33, 96), (1, 130, 112), (33, 1, 96), (130, 1, 112), (5, 7, 96), (5, 7, 112),
                                     (1, 33, 256), (33, 1, 256), (5, 7, 16), (1, 130, 64)])
def test_sequence_lstm_against_float64(tfg, B, T, U, zero_state):
    g = torch.Generator().manual_seed(B * 1000 + T + U)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    P, R = r(B * T, 4 * U), r(U, 4 * U) / np.sqrt(U)
    h0, c0 = (torch.zeros(B, U, dtype=torch.float64),) * 2 if zero_state else (r(B, U) * 0.5, r(B, U) * 0.5)
    gouts = (r(B * T, U), r(B, U), r(B, U))
    outs, grads = sequence_gpu(tfg, P, R, h0, c0, B, T, U, MASKS, gouts, zero_state)
    for mask, got in zip(MASKS, grads):
        gm = [g_ if m else None for g_, m in zip(gouts, mask)]
        ref_out, ref_g = sequence_reference(P, R, h0, c0, B, T, U, gm, torch.float64)
        cpu_out, cpu_g = sequence_reference(P, R, h0, c0, B, T, U, gm, torch.float32)
        if mask == MASKS[0]:
            for name, a, b, c in zip(("h_seq", "h_last", "c_last"), outs, ref_out, cpu_out):
                check("lstm B={} T={} U={} {}".format(B, T, U, name), a, b, c)
        for name, a, b, c in zip(("dP", "dR", "d_h0", "d_c0"), got, ref_g, cpu_g):
            check("lstm B={} T={} U={} grads{} {}".format(B, T, U, mask, name), a, b, c)


# ---- layers.LSTM against torch.nn.LSTM ----------------------------------------------------------------------------------------
def torch_lstm(F, U, kernel, R, bias, dtype):
    lstm = torch.nn.LSTM(F, U, batch_first=True).to(dtype)
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(kernel.t().to(dtype))
        lstm.weight_hh_l0.copy_(R.t().to(dtype))
        lstm.bias_ih_l0.copy_(bias.to(dtype))
        lstm.bias_hh_l0.zero_()
    return lstm


@pytest.mark.parametrize("return_sequences", [False, True])
@pytest.mark.parametrize("return_state", [False, True])
@pytest.mark.parametrize("U", [6, 20])
def test_layer_lstm_matches_torch_lstm(tfg, U, return_sequences, return_state):
    dev = tfg._lib.device()
    g = torch.Generator().manual_seed(U)
    B, T, F = 3, 4, 5
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    x, kernel, R, bias, h0, c0 = r(B, T, F), r(F, 4 * U) * 0.5, r(U, 4 * U) * 0.4, r(4 * U) * 0.3, r(1, U) * 0.5, r(B, U) * 0.5
    layer = tfg.layers.LSTM(U, return_sequences=return_sequences, return_state=return_state)
    xg, h0g, c0g = (v.float().to(dev).requires_grad_(True) for v in (x, h0, c0))
    layer._maybe_build([xg])
    layer.set_weights(kernel=kernel, recurrent_kernel=R, bias=bias)
    layer.trainable(True)
    out = layer(xg, initial_state=[h0g, c0g])
    outs = list(out) if return_state else [out]
    assert len(outs) == (3 if return_state else 1)
    gouts = [r(*o.shape) for o in outs]
    sum((o * w.float().to(dev)).sum() for o, w in zip(outs, gouts)).backward()
    got_g = [xg.grad, layer.kernel.grad, layer.recurrent_kernel.grad, layer.bias.grad, h0g.grad, c0g.grad]
    assert all(v is not None for v in got_g)

    def reference(dtype):
        lstm = torch_lstm(F, U, kernel, R, bias, dtype)
        xx, hh, cc = (v.detach().clone().to(dtype).requires_grad_(True) for v in (x, h0, c0))
        seq, (h, c) = lstm(xx, (hh.expand(B, U).unsqueeze(0).contiguous(), cc.unsqueeze(0)))
        o = [seq if return_sequences else h[0]] + ([h[0], c[0]] if return_state else [])
        sum((a * w.to(dtype)).sum() for a, w in zip(o, gouts)).backward()
        gr = [xx.grad, lstm.weight_ih_l0.grad.t(), lstm.weight_hh_l0.grad.t(), lstm.bias_ih_l0.grad, hh.grad, cc.grad]
        return [v.detach().double() for v in o], [v.double() for v in gr]

    ref_o, ref_g = reference(torch.float64)
    cpu_o, cpu_g = reference(torch.float32)
    for i, (a, b, c) in enumerate(zip(outs, ref_o, cpu_o)):
        check("layers.LSTM U={} seq={} state={} out{}".format(U, return_sequences, return_state, i), a.detach().cpu(), b, c)
    for name, a, b, c in zip(("dx", "dkernel", "drecurrent", "dbias", "dh0", "dc0"), got_g, ref_g, cpu_g):
        check("layers.LSTM U={} seq={} state={} {}".format(U, return_sequences, return_state, name), a.cpu(), b, c)


def test_lstm_layer_is_still_a_weight_holder(tfg):
    """lstm_graph_sage takes the same object and reads .kernel / .recurrent_kernel / .bias."""
    dev = tfg._lib.device()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(12, 4, generator=g).to(dev)
    ei = torch.randint(0, 12, (2, 40), generator=g).to(torch.int32).to(dev)
    layer = tfg.layers.LSTMGraphSage(8, seed=1)
    out = layer([x, ei])
    assert tuple(out.shape) == (12, 8) and bool(torch.isfinite(out).all()) and isinstance(layer.lstm, tfg.layers.LSTM)


# ---- nn.set2set / layers.Set2Set ----------------------------------------------------------------------------------------------
WEIGHTS = ("kernel", "recurrent_kernel", "bias")


def gpu_lstm(tfg, c, F, trainable):
    lstm = tfg.layers.LSTM(F, return_sequences=True, return_state=True)
    lstm._maybe_build([torch.empty(1, 1, 2 * F)])
    lstm.set_weights(**{k: np.asarray(c[k], dtype=np.float32) for k in WEIGHTS})
    return lstm.trainable(trainable)


def set2set_gpu(tfg, c, batch_graphs, grad, num_graphs=None, layer=False):
    dev = tfg._lib.device()
    F = c["x"].shape[1]
    x = torch.as_tensor(np.asarray(c["x"], dtype=np.float32)).to(dev).requires_grad_(grad)
    ids = torch.as_tensor(np.asarray(c["node_graph_index"])).to(torch.int32).to(dev)
    if layer:
        mod = tfg.layers.Set2Set(num_iterations=c["num_iterations"], batch_graphs=batch_graphs)
        mod._maybe_build([x])
        mod.lstm.set_weights(**{k: np.asarray(c[k], dtype=np.float32) for k in WEIGHTS})
        mod.trainable(grad)
        lstm = mod.lstm
        out = mod([x, ids] if num_graphs is None else [x, ids, num_graphs], cache={})
    else:
        lstm = gpu_lstm(tfg, c, F, grad)
        out = tfg.nn.set2set(x, ids, lstm, c["num_iterations"], num_graphs=num_graphs, batch_graphs=batch_graphs)
    grads = {}
    if grad:
        (out * torch.as_tensor(c["grad_out"]).float().to(dev)).sum().backward()
        grads = dict(x=x.grad.cpu(), **{k: getattr(lstm, k).grad.cpu() for k in WEIGHTS})
    return out.detach().cpu(), grads


def set2set_mirror(c, batch_graphs, grad, dtype):
    t = {k: torch.as_tensor(np.asarray(c[k], dtype=np.float64)).to(dtype).requires_grad_(grad) for k in ("x",) + WEIGHTS}
    out = M.set2set_mirror(t["x"], c["node_graph_index"], t["kernel"], t["recurrent_kernel"], t["bias"], c["num_iterations"],
                           batch_graphs=batch_graphs)
    grads = {}
    if grad:
        (out * torch.as_tensor(c["grad_out"]).to(dtype)).sum().backward()
        grads = {k: v.grad.double() for k, v in t.items()}
    return out.detach().double(), grads


@pytest.mark.parametrize("name", ["shuffled_f5_it3", "sorted_f1_it1", "shuffled_f1_it4", "one_graph_f5_it3", "sorted_f5_it1"])
def test_set2set_matches_the_reference_goldens(tfg, name):
    c = golden_cases()[name]
    ref, cpu = mirror_of_case(c), mirror_of_case(c, torch.float32)
    assert float((ref - torch.as_tensor(c["output"])).abs().max()) <= 1e-12
    gpu, _ = set2set_gpu(tfg, c, False, False)
    check("golden " + name, gpu, torch.as_tensor(c["output"]), cpu)
    gpu, _ = set2set_gpu(tfg, c, False, False, layer=True)
    check("golden layer " + name, gpu, torch.as_tensor(c["output"]), cpu)


def training_case(F, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    ids = ids[torch.randperm(ids.numel(), generator=g)]
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    G = int(ids.max()) + 1
    return dict(x=r(ids.numel(), F).numpy(), node_graph_index=ids.numpy(), kernel=(r(2 * F, 4 * F) / np.sqrt(2 * F)).numpy(),
                recurrent_kernel=(r(F, 4 * F) / np.sqrt(F)).numpy(), bias=(r(4 * F) * 0.3).numpy(), num_iterations=3,
                grad_out=r(G, 2 * F).numpy())


@pytest.mark.parametrize("batch_graphs", [False, True], ids=["literal", "per_graph"])
@pytest.mark.parametrize("F, sizes", [(5, [4, 0, 1, 30, 7]), (32, [3, CHUNK + 5, 0, 40]), (20, [9] * 37)])
def test_set2set_both_modes_forward_backward_and_determinism(tfg, F, sizes, batch_graphs):
    c = training_case(F, sizes, seed=F)
    ref, gref = set2set_mirror(c, batch_graphs, True, torch.float64)
    cpu, gcpu = set2set_mirror(c, batch_graphs, True, torch.float32)
    gpu, ggpu = set2set_gpu(tfg, c, batch_graphs, True)
    what = "set2set F={} G={} {}".format(F, len(sizes), "per-graph" if batch_graphs else "literal")
    check(what + " output", gpu, ref, cpu)
    for k in gref:
        check("{} d/d{}".format(what, k), ggpu[k], gref[k], gcpu[k])
    gpu2, ggpu2 = set2set_gpu(tfg, c, batch_graphs, True, layer=True, num_graphs=len(sizes))
    assert torch.equal(gpu, gpu2), "outputs differ between two runs (function vs layer, num_graphs derived vs given)"
    for k in ggpu:
        assert torch.equal(ggpu[k], ggpu2[k]), "d/d{} differs between two runs".format(k)


def test_set2set_num_graphs_given_adds_trailing_empty_graphs(tfg):
    c = training_case(5, [4, 2, 6], seed=2)
    derived, _ = set2set_gpu(tfg, c, True, False)
    given, _ = set2set_gpu(tfg, c, True, False, num_graphs=5)
    assert tuple(given.shape) == (5, 10) and torch.equal(given[:3], derived)
    assert float(given[3:, 5:].abs().max()) == 0.0 and torch.equal(given[3], given[4])      # empty graphs: r = 0


def test_a_reused_cache_does_not_serve_a_stale_plan(tfg):
    """One cache dict, three calls: the same ids tensor reuses the plan (no build), other ids of the same sizes and the same
    tensor modified in place rebuild it."""
    dev = tfg._lib.device()
    c = training_case(5, [4, 2, 6], seed=6)
    lstm = gpu_lstm(tfg, c, 5, False)
    x = torch.as_tensor(c["x"]).float().to(dev)
    ids = torch.as_tensor(c["node_graph_index"]).to(torch.int32).to(dev)
    cache = {}
    first = tfg.nn.set2set(x, ids, lstm, 3, num_graphs=3, cache=cache)
    builds = []
    real = tfg.plan.CsrPlan.build
    tfg.plan.CsrPlan.build = staticmethod(lambda *a, **k: builds.append(1) or real(*a, **k))
    try:
        again = tfg.nn.set2set(x, ids, lstm, 3, num_graphs=3, cache=cache)
        assert not builds and torch.equal(first, again)
        other = ids.flip(0).contiguous()
        moved = tfg.nn.set2set(x, other, lstm, 3, num_graphs=3, cache=cache)
        assert len(builds) == 1 and torch.equal(moved, tfg.nn.set2set(x, other, lstm, 3, num_graphs=3))
        other.copy_(ids)
        back = tfg.nn.set2set(x, other, lstm, 3, num_graphs=3, cache=cache)
        assert len(builds) == 3 and torch.equal(back, first)
    finally:
        tfg.plan.CsrPlan.build = real


def test_set2set_accepts_any_keras_shaped_callable(tfg):
    """`lstm` is any callable with the call shape of set2set.py:31, as gin's mlp_model: here the mirror's LSTM on the GPU."""
    dev = tfg._lib.device()
    c = training_case(5, [4, 2, 6], seed=3)
    k, r, b = (torch.as_tensor(c[n]).float().to(dev) for n in WEIGHTS)
    calls = []

    def lstm(seq, initial_state=None, training=None):
        calls.append(tuple(seq.shape))
        return M.lstm_mirror(seq, k, r, b, initial_state[0], initial_state[1])

    x = torch.as_tensor(c["x"]).float().to(dev)
    out = tfg.nn.set2set(x, torch.as_tensor(c["node_graph_index"]).to(dev), lstm, 3)
    assert calls == [(1, 3, 10)] * 3
    ref, _ = set2set_mirror(c, False, False, torch.float64)
    cpu, _ = set2set_mirror(c, False, False, torch.float32)
    check("callable lstm", out.cpu(), ref, cpu)


def test_set2set_refuses_more_than_256_features(tfg):
    dev = tfg._lib.device()
    with pytest.raises(ValueError, match="TFGX_LSTM_MAX_UNITS"):
        tfg.nn.set2set(torch.zeros(3, 257, device=dev), torch.zeros(3, dtype=torch.int32, device=dev), None, 1)


def test_demo_trains(tfg):
    """examples/demo_set2set.py: three steps, a finite and falling loss."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import demo_set2set
    losses = demo_set2set.main(steps=3, graphs=64, batch_size=64, quiet=True)
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[0] > losses[1] > losses[2]
