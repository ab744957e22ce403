# coding=utf-8
"""The LSTM GraphSAGE aggregator on the GPU (tfgx_lstm.h, nn.lstm_graph_sage, layers.LSTMGraphSage) against the float64 mirror of
tests/lstm_mirror.py, which tests/test_lstm_abi.py pins to the reference's own outputs.

Tolerance (per case and per tensor): the same mirror evaluated in float32 on the CPU is an independent f32 evaluation of the
case; the GPU result may differ from the float64 mirror by 4x that f32-CPU error (the margin covers the MFMA chain's summation
order against torch's), with a floor of 1e-6 absolute.  Every figure is printed before it is asserted.

Shapes: n_dst 1 / 33 / 130 cross the 32-row tile; U 16 .. 80 keep the recurrent kernel in LDS in both directions, 96 only in
the forward, 112 and 128 in neither; 20 and 6 are zero-padded to a multiple of 16."""
import ctypes

import numpy as np
import pytest
import torch

import lstm_mirror as M
from test_lstm_abi import golden_cases, mirror_of_case

pytestmark = pytest.mark.gpu

NAMES = ("x", "kernel", "recurrent_kernel", "lstm_bias", "self_kernel", "neighbor_kernel", "bias")


class Weights(object):
    def __init__(self, kernel, recurrent_kernel, bias):
        self.kernel, self.recurrent_kernel, self.bias = kernel, recurrent_kernel, bias


def make_case(seed, n_dst, n_src, T, U, F, concat=True, normalize=False, activation="relu", full=False):
    """Row 0 has degree T; unless `full`, the last row has degree 0 and the others random degrees; the last source row is a
    neighbour; neighbours repeat; the edge list is shuffled."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.full((n_dst,), T, dtype=torch.long) if full else torch.randint(0, T + 1, (n_dst,), generator=g)
    deg[0] = T
    if not full and n_dst > 1:
        deg[-1] = 0
    row = torch.repeat_interleave(torch.arange(n_dst), deg)
    col = torch.randint(0, n_src, (int(deg.sum()),), generator=g)
    col[0] = n_src - 1
    p = torch.randperm(row.numel(), generator=g)
    ei = torch.stack([row[p], col[p]]).to(torch.int32)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    ku = U
    c = dict(x=r(n_src, F), edge_index=ei, kernel=r(F, 4 * U) / np.sqrt(F), recurrent_kernel=r(U, 4 * U) / np.sqrt(U),
             lstm_bias=r(4 * U) * 0.3, self_kernel=r(F, ku) / np.sqrt(F), neighbor_kernel=r(ku, ku) / np.sqrt(ku),
             bias=r(2 * ku if concat else ku) * 0.2, concat=concat, normalize=normalize, activation=activation, n_dst=n_dst)
    return c


def run_mirror(c, dtype, grad):
    t = {k: (None if c.get(k) is None else torch.as_tensor(np.asarray(c[k], dtype=np.float64)).to(dtype).requires_grad_(grad))
         for k in NAMES}
    out = M.lstm_sage_mirror(t["x"], c["edge_index"], t["kernel"], t["recurrent_kernel"], t["lstm_bias"], t["self_kernel"],
                             t["neighbor_kernel"], t["bias"], c["activation"], c["concat"], c["normalize"], n_dst=c.get("n_dst"))
    grads = {}
    if grad:
        gw = torch.as_tensor(c["grad_out"]).to(dtype)
        (out * gw).sum().backward()
        grads = {k: v.grad.double() for k, v in t.items() if v is not None}
    return out.detach().double(), grads


def run_gpu(tfg, c, grad):
    dev = tfg._lib.device()
    t = {k: (None if c.get(k) is None else torch.as_tensor(np.asarray(c[k], dtype=np.float32)).to(dev).requires_grad_(grad))
         for k in NAMES}
    ei = torch.as_tensor(np.asarray(c["edge_index"])).to(dev)
    n_dst, n_src = c.get("n_dst") or t["x"].shape[0], t["x"].shape[0]
    cache = {}
    if n_dst != n_src:
        cache[tfg.plan.CACHE_KEY_PLAN] = tfg.plan.CsrPlan.build(ei, n_dst, n_src)
    act = tfg.activations.relu if c["activation"] == "relu" else None
    out = tfg.nn.lstm_graph_sage(t["x"], ei, Weights(t["kernel"], t["recurrent_kernel"], t["lstm_bias"]), t["self_kernel"],
                                 t["neighbor_kernel"], bias=t["bias"], activation=act, concat=c["concat"],
                                 normalize=c["normalize"], cache=cache)
    grads = {}
    if grad:
        (out * torch.as_tensor(c["grad_out"]).to(dev).float()).sum().backward()
        grads = {k: v.grad.detach().double().cpu() for k, v in t.items() if v is not None}
    return out.detach().double().cpu(), grads


def check(what, gpu, ref, cpu32):
    cpu_err = float((cpu32 - ref).abs().max())
    gpu_err = float((gpu - ref).abs().max())
    tol = max(4.0 * cpu_err, 1e-6)
    print("{}: cpu-f32 err {:.3e}  gpu err {:.3e}  tol {:.3e}".format(what, cpu_err, gpu_err, tol))
    assert gpu.shape == ref.shape, what
    assert gpu_err <= tol, "{}: gpu err {:.3e} > tol {:.3e} (cpu-f32 err {:.3e})".format(what, gpu_err, tol, cpu_err)


def compare(tfg, c, grad, what):
    if grad:
        n_out = (c.get("n_dst") or c["x"].shape[0], c["neighbor_kernel"].shape[1] * (2 if c["concat"] else 1))
        c["grad_out"] = torch.randn(*n_out, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    ref, gref = run_mirror(c, torch.float64, grad)
    cpu, gcpu = run_mirror(c, torch.float32, grad)
    gpu, ggpu = run_gpu(tfg, c, grad)
    check(what + " output", gpu, ref, cpu)
    for k in gref:
        assert k in ggpu and ggpu[k] is not None, "{}: no gradient for {}".format(what, k)
        check("{} d/d{}".format(what, k), ggpu[k], gref[k], gcpu[k])
    return gpu, ggpu


# (n_dst, n_src, T, U, F, concat, normalize, activation, full)
SWEEP = [
    (1, 1, 1, 16, 1, True, False, "relu", True),
    (33, 33, 2, 48, 5, False, False, None, False),
    (130, 130, 7, 64, 100, True, True, "relu", False),
    (33, 57, 7, 80, 5, True, False, None, False),        # n_src != n_dst; resident in both directions
    (130, 130, 2, 96, 5, False, True, None, True),       # resident forward, streamed backward; every row of degree T
    (33, 40, 7, 112, 100, True, False, "relu", False),   # streamed in both
    (130, 130, 1, 128, 1, True, False, None, False),
    (33, 33, 7, 20, 5, False, False, "relu", False),     # zero-padded to 32
    (1, 9, 2, 256, 5, True, False, None, True),          # the largest U
]


@pytest.mark.parametrize("name", ["concat", "add", "concat_normalize", "add_normalize"])
def test_forward_matches_the_reference_goldens(tfg, name):
    c = golden_cases()[name]
    ref, cpu = mirror_of_case(c), mirror_of_case(c, torch.float32).double()
    gpu, _ = run_gpu(tfg, c, False)
    assert float((ref - torch.as_tensor(c["output"])).abs().max()) <= 1e-12
    check("golden " + name, gpu, torch.as_tensor(c["output"]), cpu)


@pytest.mark.parametrize("shape", SWEEP, ids=lambda s: "n{}_s{}_T{}_U{}_F{}".format(*s[:5]))
def test_forward_sweep(tfg, shape):
    n_dst, n_src, T, U, F, concat, normalize, act, full = shape
    c = make_case(11, n_dst, n_src, T, U, F, concat, normalize, act, full)
    compare(tfg, c, False, "fwd {}".format(shape[:5]))


@pytest.mark.parametrize("shape", SWEEP, ids=lambda s: "n{}_s{}_T{}_U{}_F{}".format(*s[:5]))
def test_backward_sweep_and_determinism(tfg, shape):
    n_dst, n_src, T, U, F, concat, normalize, act, full = shape
    c = make_case(12, n_dst, n_src, T, U, F, concat, normalize, act, full)
    out1, g1 = compare(tfg, c, True, "bwd {}".format(shape[:5]))
    out2, g2 = run_gpu(tfg, c, True)
    assert torch.equal(out1, out2), "forward differs between two runs"
    for k in g1:
        assert torch.equal(g1[k], g2[k]), "d/d{} differs between two runs".format(k)


def test_no_edges_gives_a_zero_neighbour_term(tfg):
    c = make_case(3, 5, 5, 1, 16, 3, concat=True, activation=None)
    c["edge_index"] = torch.zeros((2, 0), dtype=torch.int32)
    gpu, _ = run_gpu(tfg, c, False)
    assert float(gpu[:, 16:].sub(torch.as_tensor(c["bias"])[16:]).abs().max()) <= 1e-6


def test_too_many_units_is_refused(tfg):
    c = make_case(3, 2, 2, 1, 260, 2)
    with pytest.raises(NotImplementedError, match="256"):
        run_gpu(tfg, c, False)


def test_bad_col_through_the_raw_abi(tfg):
    """A valid buffer holding an out-of-range VALUE: the step is a pad step and the flag is raised; so is a row longer than T
    (truncated).  The clean call leaves the flag at 0."""
    L = tfg._lib
    lib, dev = L.require_gpu(), L.device()
    g = torch.Generator().manual_seed(4)
    n_dst, n_src, T, U = 5, 6, 3, 16
    row_ptr = torch.tensor([0, 3, 3, 5, 6, 8], dtype=torch.int32)
    col = torch.tensor([1, 5, 0, 2, 2, 4, 3, 0], dtype=torch.int32)
    P, p_pad = torch.randn(n_src, 4 * U, generator=g, dtype=torch.float64), torch.randn(4 * U, generator=g, dtype=torch.float64)
    R = torch.randn(U, 4 * U, generator=g, dtype=torch.float64) / 4.0

    def launch(col_, T_):
        d = lambda t, dt=torch.float32: t.to(dt).to(dev).contiguous()      # noqa: E731
        rp, cc, Pd, pd, Rd = d(row_ptr, torch.int32), d(col_, torch.int32), d(P), d(p_pad), d(R)
        out = torch.empty((n_dst, U), dtype=torch.float32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        L.check(lib.tfgx_lstm_aggregate_f32(L.ptr(rp), L.ptr(cc), n_dst, n_src, T_, L.ptr(Pd), 4 * U, L.ptr(pd), L.ptr(Rd), U,
                                            L.ptr(out), U, None, 0, L.ptr(flag), L.stream_ptr()), "tfgx_lstm_aggregate_f32")
        return out.double().cpu(), int(flag.item())

    def mirror(col_, T_):
        nbr = torch.full((n_dst, T_), -1, dtype=torch.long)
        for i in range(n_dst):
            for t in range(min(T_, int(row_ptr[i + 1] - row_ptr[i]))):
                j = int(col_[int(row_ptr[i]) + t])
                nbr[i, t] = j if 0 <= j < n_src else -1
        return (M.aggregate_mirror(P, p_pad, R, nbr), M.aggregate_mirror(P.float(), p_pad.float(), R.float(), nbr).double())

    out, flag = launch(col, T)
    assert flag == 0
    check("clean", out, *mirror(col, T))
    for bad_value in (n_src, -1, 2 ** 31 - 1):
        bad = col.clone()
        bad[4] = bad_value
        out, flag = launch(bad, T)
        assert flag == 1
        check("bad col {}".format(bad_value), out, *mirror(bad, T))
    out, flag = launch(col, 2)          # row 0 has 3 edges: truncated to T = 2
    assert flag == 1
    check("truncated", out, *mirror(col, 2))


def test_sampler_hand_off(tfg):
    """A sampled edge list carries its plan: from_cache returns it, no second plan is built."""
    dev = tfg._lib.device()
    g = torch.Generator().manual_seed(8)
    n = 60
    ei = torch.randint(0, n, (2, 600), generator=g).to(torch.int32).to(dev)
    sampled, _ = tfg.utils.RandomNeighborSampler(ei).sample(k=5, seed=3)
    attached = sampled._tfgx_plan
    cache = {}
    assert tfg.plan.CsrPlan.from_cache(sampled, n, n, cache).row_ptr.data_ptr() == attached.padded_to(n, n).row_ptr.data_ptr() \
        or tfg.plan.CsrPlan.from_cache(sampled, n, n, cache) is attached
    builds = []
    real = tfg.plan.CsrPlan.build
    tfg.plan.CsrPlan.build = staticmethod(lambda *a, **k: builds.append(1) or real(*a, **k))
    try:
        c = make_case(5, n, n, 5, 32, 7)
        c["edge_index"] = sampled.cpu()
        ref, _ = run_mirror(c, torch.float64, False)
        cpu, _ = run_mirror(c, torch.float32, False)
        t = {k: torch.as_tensor(np.asarray(c[k], dtype=np.float32)).to(dev) for k in NAMES}
        out = tfg.nn.lstm_graph_sage(t["x"], sampled, Weights(t["kernel"], t["recurrent_kernel"], t["lstm_bias"]),
                                     t["self_kernel"], t["neighbor_kernel"], bias=t["bias"], activation=tfg.activations.relu)
    finally:
        tfg.plan.CsrPlan.build = real
    assert not builds, "a second plan was built for a sampled edge list"
    assert tfg.autograd.lstm_max_degree(tfg.plan.CsrPlan.from_cache(sampled, n, n, None)) <= 5
    check("sampled", out.double().cpu(), ref, cpu)


def test_layer_trains(tfg):
    """LSTMGraphSage(32) on a 200-node graph: three SGD steps, the loss is finite and decreases."""
    dev = tfg._lib.device()
    g = torch.Generator().manual_seed(21)
    n, F = 200, 12
    x = torch.randn(n, F, generator=g).to(dev)
    ei = torch.randint(0, n, (2, 1200), generator=g).to(torch.int32).to(dev)
    y = torch.randn(n, 32, generator=g).to(dev)
    layer = tfg.layers.LSTMGraphSage(32, seed=1).trainable(True)
    cache = {}
    layer([x, ei], cache=cache)
    params = layer.parameters()
    assert len(params) == 6 and all(p.requires_grad for p in params)
    assert float(layer.lstm.bias[16:32].min()) == 1.0 and float(layer.lstm.bias[:16].abs().max()) == 0.0     # unit_forget_bias
    opt = torch.optim.SGD(params, lr=0.05)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = ((layer([x, ei, None], cache=cache, training=True) - y) ** 2).mean()
        loss.backward()
        assert all(p.grad is not None for p in params)
        opt.step()
        losses.append(float(loss))
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[0] > losses[1] > losses[2]
