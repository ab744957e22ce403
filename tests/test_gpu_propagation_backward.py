# coding=utf-8
"""The TRAINING path of the seven propagation convolutions (nn/conv/propagation.py: GIN, SGC, TAGCN, APPNP, SSGC, ChebyNet,
LEConv) against float64 autograd of tests/propagation_mirror.py, which tests/test_propagation_mirror.py pins to the reference.

Per case, with leaf tensors that require grad: (1) the training-path forward, (2) EVERY gradient under a fixed random upstream G
(a missing one is a failure), (3) the inference-path forward of the same call (torch.no_grad(), no leaf tracked) — all three
against the same float64 mirror at the same bar, so the two routes are shown to agree and every shape-picked rewrite (TAGCN's
Horner / concat, ChebyNet's Clenshaw / literal recurrence, SGC's commuted GEMM) is compared with a reference on dense x.

The bar (per tensor, measured, as test_gpu_lstm_sage.check does it): the same mirror in float32 on the CPU is an independent
float32 evaluation; the GPU may differ from the float64 mirror by 4x that float32 error (summation order), floor
1e-6 * max(1, max|ref|).  The un-normalised ChebyNet works with degree-sized values and the bar scales with them by itself.
Cases flagged `rewritten_bar` take the larger of the literal and the rewritten-order float32 errors (REWRITTEN_BAR below says
which and why); the float64 reference is always the literal order.  Every figure is printed before it is asserted.

ReLU kinks: entries of G whose float64 output pre-activation lies within 1e-4 of zero are zeroed (f64_layers' G_eff rule; at most
1 % of G, asserted); hidden ReLUs (the APPNP / SSGC encoder, GIN's MLP) cannot be isolated by G, so each such case's seed was
chosen on the CPU so that no hidden float64 pre-activation lies within 1e-4 of zero — asserted here.

One small directed graph (propagation_mirror.structured_graph): these layers go wrong at structure, not at size."""
import numpy as np
import pytest
import torch

import propagation_mirror as M
import reference_cases as RC

pytestmark = pytest.mark.gpu

KINK = 1e-4
GRAPH = M.structured_graph()
N, F, EI, W = GRAPH["n"], GRAPH["f"], GRAPH["ei"], GRAPH["w"]

# cases whose bar also takes the float32 error of the rewritten association: none needed it (measured on an MI355X: the worst
# gpu_err / tol of any tensor of any case is 0.39, appnp-k6-mlp's training forward; every rewritten branch sits below 0.28)
REWRITTEN_BAR = set()

# seeds of the cases with hidden ReLUs, searched on the CPU from 100 upwards for a float64 mirror without a hidden
# pre-activation within 3 * KINK of zero (the first seed tried holds for all six: smallest |pre| 6.8e-4 .. 8.1e-4; the test
# asserts > KINK); every other case takes DEFAULT_SEED
DEFAULT_SEED = 100
SEEDS = {"appnp-k6-mlp": 100, "appnp-k0": 100, "ssgc-k5-mlp": 100, "sparse-x-appnp": 100, "gin-eps": 100, "gin-layer-train-eps": 100}


class Case(object):
    def __init__(self, name, p, mirror, gpu, const=None, frozen=(), rewritten=False):
        self.name, self.p, self.mirror, self.gpu = name, p, mirror, gpu
        self.const, self.frozen, self.rewritten = dict(const or {}), set(frozen), rewritten
        self.rewritten_bar = name in REWRITTEN_BAR


def _rng(name):
    return np.random.Generator(np.random.PCG64(SEEDS.get(name, DEFAULT_SEED)))


def _x(rng):
    return rng.standard_normal((N, F), dtype=np.float32)


def _sparse_table(rng):
    dense = ((rng.random((N, F)) < 0.3) * rng.standard_normal((N, F))).astype(np.float32)
    dense[3] = 0
    return dense


def _as_sparse(tfg, dense):
    r, c = np.nonzero(dense)
    return tfg.SparseMatrix(np.stack([r, c]).astype(np.int32), dense[r, c], [N, F])


def _relu(tfg, a):
    return None if a is None else tfg.relu


# ---- the case table ----------------------------------------------------------------------------------------------------------
def _sgc(name, k, units, sparse=False, **cfg):
    rng = _rng(name)
    x = _sparse_table(rng) if sparse else _x(rng)
    p = dict(kernel=RC.glorot(rng, F, units), bias=RC.small_bias(rng, units))
    const = {}
    if sparse:
        const["x"] = x
    else:
        p = dict(x=x, **p)

    def mirror(t, dtype, order, tap):
        return M.sgc(t.get("x", const.get("x")), EI, W, k, t["kernel"], t["bias"], "relu", dtype=dtype, order=order, tap=tap, **cfg)

    def gpu(tfg, t, cache):
        xx = _as_sparse(tfg, const["x"]) if sparse else t["x"]
        return tfg.nn.sgc(xx, EI, W, k, t["kernel"], t["bias"], tfg.relu, cache=cache, **cfg)
    return Case(name, p, mirror, gpu, const, rewritten=(not sparse and units > F))


def _tagcn(name, k, units):
    rng = _rng(name)
    p = dict(x=_x(rng), kernel=RC.glorot(rng, F * (k + 1), units), bias=RC.small_bias(rng, units))

    def mirror(t, dtype, order, tap):
        return M.tagcn(t["x"], EI, W, k, t["kernel"], t["bias"], "relu", dtype=dtype, order=order, tap=tap)

    def gpu(tfg, t, cache):
        return tfg.nn.tagcn(t["x"], EI, W, k, t["kernel"], t["bias"], tfg.relu, cache=cache)
    return Case(name, p, mirror, gpu, rewritten=units < F)


def _mlp_params(rng, p, widths):
    last = F
    for i, u in enumerate(widths):
        p["kernel_{}".format(i)], p["bias_{}".format(i)] = RC.glorot(rng, last, u), RC.small_bias(rng, u)
        last = u


def _lists(t, n):
    if n == 0:
        return None, None
    return [t["kernel_{}".format(i)] for i in range(n)], [t["bias_{}".format(i)] for i in range(n)]


def _mlp_prop(name, fn, k, alpha, widths, activation=None, sparse=False):
    """fn: "appnp" or "ssgc"; widths: the encoder's units ([] = kernels None, x is the propagated signal)."""
    rng = _rng(name)
    x = _sparse_table(rng) if sparse else _x(rng)
    p, const = {}, {}
    if sparse:
        const["x"] = x
    else:
        p["x"] = x
    _mlp_params(rng, p, widths)
    nw = len(widths)

    def mirror(t, dtype, order, tap):
        ks, bs = _lists(t, nw)
        return getattr(M, fn)(t.get("x", const.get("x")), EI, W, ks, bs, k=k, alpha=alpha, activation=activation, dtype=dtype,
                              order=order, tap=tap)

    def gpu(tfg, t, cache):
        ks, bs = _lists(t, nw)
        xx = _as_sparse(tfg, const["x"]) if sparse else t["x"]
        return getattr(tfg.nn, fn)(xx, EI, W, ks, bs, k=k, alpha=alpha, activation=_relu(tfg, activation), cache=cache)
    return Case(name, p, mirror, gpu, const)


def _cheb(name, norm, k, units, dynamic=False, sparse=False):
    rng = _rng(name)
    x = _sparse_table(rng) if sparse else _x(rng)
    p, const = {}, {}
    if sparse:
        const["x"] = x
    else:
        p["x"] = x
    for i in range(k):
        p["kernel{}".format(i)] = RC.glorot(rng, F, units)
    p["bias"] = RC.small_bias(rng, units)

    def mirror(t, dtype, order, tap):
        return M.chebynet(t.get("x", const.get("x")), EI, W, k, [t["kernel{}".format(i)] for i in range(k)], t["bias"], "relu",
                          norm, dynamic, dtype=dtype, order=order, tap=tap)

    def gpu(tfg, t, cache):
        xx = _as_sparse(tfg, const["x"]) if sparse else t["x"]
        return tfg.nn.chebynet(xx, EI, W, k, [t["kernel{}".format(i)] for i in range(k)], t["bias"], tfg.relu, norm, dynamic,
                               cache=cache)
    return Case(name, p, mirror, gpu, const, rewritten=(not sparse and k >= 2 and units < F))


def _gin(name, through_layer):
    rng = _rng(name)
    p = dict(x=_x(rng), eps=np.float32(0.3), w1=RC.glorot(rng, F, 8), b1=RC.small_bias(rng, 8), w2=RC.glorot(rng, 8, 5))

    def mirror(t, dtype, order, tap):
        def mlp(h):
            pre = h @ t["w1"] + t["b1"]
            tap.setdefault("hidden", []).append(pre)
            return torch.relu(pre) @ t["w2"]
        return M.gin(t["x"], EI, mlp, t["eps"], dtype=dtype)

    def gpu(tfg, t, cache):
        mlp = lambda h, training=None: torch.relu(h @ t["w1"] + t["b1"]) @ t["w2"]      # noqa: E731
        if not through_layer:
            return tfg.nn.gin(t["x"], EI, mlp, t["eps"], cache=cache)
        layer = tfg.layers.GIN(mlp, eps=7.0, train_eps=True)        # train_eps: the weight replaces the constructor's eps
        layer._maybe_build([t["x"]])
        layer.set_weights(eps=t["eps"].detach())
        layer.trainable(t["eps"].requires_grad)
        assert [tuple(q.shape) for q in layer.parameters()] == [()] and layer.parameters()[0] is layer.eps
        t["eps"] = layer.eps
        return layer([t["x"], EI], cache=cache)
    return Case(name, p, mirror, gpu)


def _le_conv(name, weighted, biases, w_leaf=False, frozen=()):
    rng = _rng(name)
    p = dict(x=_x(rng))
    for tag, has in zip(("self", "aggr_self", "aggr_neighbor"), biases):
        p[tag + "_kernel"] = RC.glorot(rng, F, 6)
        if has:
            p[tag + "_bias"] = RC.small_bias(rng, 6)
    if w_leaf:
        p["edge_weight"] = W.copy()

    def args(t):
        w = t["edge_weight"] if w_leaf else (W if weighted else None)
        return (t["x"], EI, w, t["self_kernel"], t.get("self_bias"), t["aggr_self_kernel"], t.get("aggr_self_bias"),
                t["aggr_neighbor_kernel"], t.get("aggr_neighbor_bias"))

    def mirror(t, dtype, order, tap):
        return M.le_conv(*args(t), activation="relu", dtype=dtype, tap=tap)

    def gpu(tfg, t, cache):
        return tfg.nn.le_conv(*args(t), activation=tfg.relu, cache=cache)
    return Case(name, p, mirror, gpu, frozen=frozen)


BUILDERS = {
    "sgc-k1": lambda n: _sgc(n, 1, 9),
    "sgc-k3": lambda n: _sgc(n, 3, 9),
    "sgc-k2-widening": lambda n: _sgc(n, 2, 30),
    "sgc-renorm-false": lambda n: _sgc(n, 2, 9, renorm=False),
    "sgc-improved": lambda n: _sgc(n, 2, 9, improved=True),
    "tagcn-k3-units7-horner": lambda n: _tagcn(n, 3, 7),
    "tagcn-k3-units20-concat": lambda n: _tagcn(n, 3, 20),
    "tagcn-k1": lambda n: _tagcn(n, 1, 7),
    "appnp-k6-mlp": lambda n: _mlp_prop(n, "appnp", 6, 0.15, [16, 6]),
    "appnp-k0": lambda n: _mlp_prop(n, "appnp", 0, 0.15, [16, 6]),
    "appnp-no-mlp": lambda n: _mlp_prop(n, "appnp", 4, 0.15, [], activation="relu"),
    "ssgc-k5-mlp": lambda n: _mlp_prop(n, "ssgc", 5, 0.2, [16, 6]),
    "ssgc-plain": lambda n: _mlp_prop(n, "ssgc", 4, 0.1, []),
    "chebynet-sym-dynamic": lambda n: _cheb(n, "sym", 3, 5, dynamic=True),
    "gin-eps": lambda n: _gin(n, False),
    "gin-layer-train-eps": lambda n: _gin(n, True),
    "le_conv-weighted-three-biases": lambda n: _le_conv(n, True, (True, True, True)),
    "le_conv-unweighted": lambda n: _le_conv(n, False, (True, True, False)),
    "le_conv-edge-weight-grad": lambda n: _le_conv(n, True, (True, True, True), w_leaf=True),
    "le_conv-only-edge-weight-tracked": lambda n: _le_conv(
        n, True, (True, False, False), w_leaf=True,
        frozen=("x", "self_kernel", "self_bias", "aggr_self_kernel", "aggr_neighbor_kernel")),
    "sparse-x-sgc": lambda n: _sgc(n, 2, 9, sparse=True),
    "sparse-x-appnp": lambda n: _mlp_prop(n, "appnp", 4, 0.1, [16, 6], sparse=True),
    "sparse-x-chebynet": lambda n: _cheb(n, "sym", 3, 8, sparse=True),
}
for _norm in ("sym", "rw", None):
    for _k in (1, 2, 4):
        for _u in (5, 16):
            BUILDERS["chebynet-{}-k{}-units{}".format(_norm, _k, _u)] = \
                (lambda norm, k, u: lambda n: _cheb(n, norm, k, u))(_norm, _k, _u)


# ---- the runners -------------------------------------------------------------------------------------------------------------
def run_mirror(case, dtype, order="literal", G_eff=None):
    """-> (out, grads, tap, G, G_eff).  Without G_eff (the float64 run): a fixed random G is drawn and the entries at this
    run's own output kink are zeroed; the float32 runs are handed that G_eff."""
    t = {k: torch.as_tensor(np.asarray(v, np.float64)).to(dtype).requires_grad_(True) for k, v in case.p.items()}
    tap = {}
    out = case.mirror(t, dtype, order, tap)
    G = None
    if G_eff is None:
        G = torch.randn(out.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
        G_eff = G * (tap["pre"].detach().abs() > KINK) if "pre" in tap else G      # no output activation: nothing to zero
    out.backward(G_eff.to(dtype))
    grads = {k: (None if v.grad is None else v.grad.double()) for k, v in t.items() if k not in case.frozen}
    return out.detach().double(), grads, tap, G, G_eff


def run_gpu(tfg, case, G_eff, train):
    dev = tfg._lib.device()
    t = {k: torch.as_tensor(np.asarray(v, np.float32)).to(dev).requires_grad_(train and k not in case.frozen)
         for k, v in case.p.items()}
    if not train:
        with torch.no_grad():
            return case.gpu(tfg, t, {}).double().cpu(), {}
    out = case.gpu(tfg, t, {})
    out.backward(G_eff.float().to(dev))
    grads = {k: (None if v.grad is None else v.grad.detach().double().cpu()) for k, v in t.items() if k not in case.frozen}
    return out.detach().double().cpu(), grads


def bar(ref, errs32):
    return max(4.0 * max(errs32), 1e-6 * max(1.0, float(ref.abs().max())))


def check(what, gpu, ref, cpu32, cpu32_rewritten, use_rewritten, failures):
    """Prints the figures, records a failure instead of raising (every tensor of the case is reported), returns gpu_err / tol."""
    assert gpu.shape == ref.shape, "{}: shape {} vs {}".format(what, tuple(gpu.shape), tuple(ref.shape))
    e_lit = float((cpu32 - ref).abs().max())
    e_rw = None if cpu32_rewritten is None else float((cpu32_rewritten - ref).abs().max())
    gpu_err = float((gpu - ref).abs().max())
    tol = bar(ref, [e_lit] + ([e_rw] if (use_rewritten and e_rw is not None) else []))
    print("{}: max|ref| {:.3e}  cpu-f32 err {:.3e}  rewritten-f32 err {}  gpu err {:.3e}  tol {:.3e}  ratio {:.3f}".format(
        what, float(ref.abs().max()), e_lit, "-" if e_rw is None else "{:.3e}".format(e_rw), gpu_err, tol, gpu_err / tol))
    if not gpu_err <= tol:
        failures.append("{}: gpu err {:.3e} > tol {:.3e}".format(what, gpu_err, tol))
    return gpu_err / tol


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_training_and_inference_paths_match_float64_autograd(tfg, name):
    case = BUILDERS[name](name)
    ref, gref, tap, G, G_eff = run_mirror(case, torch.float64)
    zeroed = float(((G_eff == 0) & (G != 0)).double().mean())
    hidden_margin = min([float(h.detach().abs().min()) for h in tap.get("hidden", [])] or [float("inf")])
    print("{}: seed {}  G entries zeroed at the output kink {:.4%}  smallest hidden |pre| {:.3e}".format(
        name, SEEDS.get(name, DEFAULT_SEED), zeroed, hidden_margin))
    assert zeroed <= 0.01
    assert hidden_margin > KINK, "a hidden pre-activation sits on the ReLU kink: choose another seed for this case on the CPU"
    cpu, gcpu = run_mirror(case, torch.float32, G_eff=G_eff)[:2]
    rw, grw = (None, {})
    if case.rewritten:
        rw, grw = run_mirror(case, torch.float32, order="rewritten", G_eff=G_eff)[:2]
    out_train, ggpu = run_gpu(tfg, case, G_eff, True)
    out_infer, _ = run_gpu(tfg, case, G_eff, False)
    failures, ratios = [], {}
    ratios["forward (training path)"] = check(name + " forward (training path)", out_train, ref, cpu, rw, case.rewritten_bar, failures)
    ratios["forward (inference path)"] = check(name + " forward (inference path)", out_infer, ref, cpu, rw, case.rewritten_bar, failures)
    assert sorted(gref) == sorted(k for k in case.p if k not in case.frozen)
    for k in sorted(gref):
        assert gref[k] is not None, "the mirror has no gradient for " + k
        if ggpu.get(k) is None:
            failures.append("{}: no gradient for {}".format(name, k))
            continue
        ratios["d/d" + k] = check("{} d/d{}".format(name, k), ggpu[k], gref[k], gcpu[k], grw.get(k), case.rewritten_bar, failures)
    worst = max(ratios, key=ratios.get)
    print("RATIO {} worst gpu_err/tol {:.3f} ({}){}".format(name, ratios[worst], worst, "  [rewritten-order bar]" if case.rewritten_bar else ""))
    assert not failures, "\n".join(failures)


# ---- a trainable edge_weight on the normalised layers is refused, never dropped ----------------------------------------------------
def _normalised_calls(tfg, x, k9, ks, bs, ck):
    nn = tfg.nn
    return {
        "sgc": lambda w, c: nn.sgc(x, EI, w, 2, k9, cache=c),
        "tagcn": lambda w, c: nn.tagcn(x, EI, w, 2, torch.cat([k9, k9, k9]), cache=c),
        "appnp": lambda w, c: nn.appnp(x, EI, w, ks, bs, k=2, cache=c),
        "ssgc": lambda w, c: nn.ssgc(x, EI, w, ks, bs, k=2, cache=c),
        "chebynet-sym": lambda w, c: nn.chebynet(x, EI, w, 2, ck, cache=c),
        "chebynet-None": lambda w, c: nn.chebynet(x, EI, w, 2, ck, normalization_type=None, cache=c),
    }


@pytest.mark.parametrize("which", ["sgc", "tagcn", "appnp", "ssgc", "chebynet-sym", "chebynet-None"])
def test_trainable_edge_weight_is_refused_not_dropped(tfg, which):
    dev = tfg._lib.device()
    rng = np.random.Generator(np.random.PCG64(3))
    d = lambda a: torch.as_tensor(a).to(dev)      # noqa: E731
    x, k9 = d(_x(rng)), d(RC.glorot(rng, F, 9))
    ks, bs = [d(RC.glorot(rng, F, 8)), d(RC.glorot(rng, 8, 4))], [d(RC.small_bias(rng, 8)), d(RC.small_bias(rng, 4))]
    ck = [d(RC.glorot(rng, F, 5)), d(RC.glorot(rng, F, 5))]
    call = _normalised_calls(tfg, x, k9, ks, bs, ck)[which]
    w = d(W).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="edge_weight"):
        call(w, None)
    cache = {}
    plain = call(w.detach(), cache)                 # fills the cache (adjacency, normalised adjacency / Laplacian)
    assert cache
    with pytest.raises(NotImplementedError, match="edge_weight"):
        call(w, cache)                              # a cached adjacency must not hide it
    with torch.no_grad():
        assert torch.equal(call(w, None), plain)    # grad mode off: nothing to drop
    x.requires_grad_(True)                          # another tracked leaf changes nothing about the refusal
    with pytest.raises(NotImplementedError, match="edge_weight"):
        call(w, cache)
    x.requires_grad_(False)


# ---- dropout arguments at inference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["appnp", "ssgc"])
@pytest.mark.parametrize("tracked", [False, True], ids=["inference-path", "training-path"])
def test_dropout_rates_do_nothing_when_not_training(tfg, fn, tracked):
    dev = tfg._lib.device()
    rng = np.random.Generator(np.random.PCG64(4))
    d = lambda a: torch.as_tensor(a).to(dev).requires_grad_(tracked)      # noqa: E731
    x = torch.as_tensor(_x(rng)).to(dev)
    ks, bs = [d(RC.glorot(rng, F, 16)), d(RC.glorot(rng, 16, 6))], [d(RC.small_bias(rng, 16)), d(RC.small_bias(rng, 6))]
    f = getattr(tfg.nn, fn)
    base = f(x, EI, W, ks, bs, k=3, alpha=0.15, training=False)
    for rates in (dict(dense_drop_rate=0.5), dict(last_dense_drop_rate=0.5), dict(edge_drop_rate=0.5),
                  dict(dense_drop_rate=0.3, last_dense_drop_rate=0.4, edge_drop_rate=0.6)):
        got = f(x, EI, W, ks, bs, k=3, alpha=0.15, training=False, **rates)
        assert torch.equal(got, base), "{} {}: output changed with training=False".format(fn, rates)
    layer_cls = getattr(tfg.layers, fn.upper())
    quiet, noisy = layer_cls([16, 6], k=3, alpha=0.15), layer_cls([16, 6], k=3, alpha=0.15, dense_drop_rate=0.5,
                                                                  last_dense_drop_rate=0.5, edge_drop_rate=0.5)
    for layer in (quiet, noisy):
        layer._maybe_build([x])
        layer.set_weights(kernel_0=ks[0], bias_0=bs[0], kernel_1=ks[1], bias_1=bs[1])
        layer.trainable(tracked)
    assert torch.equal(quiet([x, EI, W]), noisy([x, EI, W]))
    assert torch.equal(quiet([x, EI, W], training=False), noisy([x, EI, W], training=False))
    assert torch.equal(quiet([x, EI, W]), base)


# ---- the layer classes hand every weight to autograd -----------------------------------------------------------------------------
def _layer_specs(tfg, rng):
    """(name, layer, weights by the reference's variable names, the nn.* call over a dict of those names)."""
    nn, relu = tfg.nn, tfg.relu
    g, b = lambda a, c: RC.glorot(rng, a, c), lambda u: RC.small_bias(rng, u)      # noqa: E731
    mlp_w = torch.as_tensor(g(F, 8)).to(tfg._lib.device())
    mlp = lambda h, training=None: torch.relu(h @ mlp_w)      # noqa: E731
    mk = dict(kernel_0=g(F, 16), bias_0=b(16), kernel_1=g(16, 6), bias_1=b(6))
    mlp_lists = lambda t: ([t["kernel_0"], t["kernel_1"]], [t["bias_0"], t["bias_1"]])      # noqa: E731
    le = dict(self_kernel=g(F, 6), self_bias=b(6), aggr_self_kernel=g(F, 6), aggr_self_bias=b(6), aggr_neighbor_kernel=g(F, 6),
              aggr_neighbor_bias=b(6))
    return [
        ("SGC", tfg.layers.SGC(9, k=2, activation=relu), dict(kernel=g(F, 9), bias=b(9)),
         lambda x, t: nn.sgc(x, EI, W, 2, t["kernel"], t["bias"], relu)),
        ("TAGCN", tfg.layers.TAGCN(7, k=3, activation=relu), dict(kernel=g(F * 4, 7), bias=b(7)),
         lambda x, t: nn.tagcn(x, EI, W, 3, t["kernel"], t["bias"], relu)),
        ("APPNP", tfg.layers.APPNP([16, 6], k=3, alpha=0.15), dict(mk),
         lambda x, t: nn.appnp(x, EI, W, *mlp_lists(t), k=3, alpha=0.15)),
        ("SSGC", tfg.layers.SSGC([16, 6], k=3, alpha=0.2), dict(mk),
         lambda x, t: nn.ssgc(x, EI, W, *mlp_lists(t), k=3, alpha=0.2)),
        ("ChebyNet", tfg.layers.ChebyNet(5, 3, activation=relu), dict(kernel0=g(F, 5), kernel1=g(F, 5), kernel2=g(F, 5), bias=b(5)),
         lambda x, t: nn.chebynet(x, EI, W, 3, [t["kernel0"], t["kernel1"], t["kernel2"]], t["bias"], relu)),
        ("LEConv", tfg.layers.LEConv(6, activation=relu, aggr_neighbor_use_bias=True), le,
         lambda x, t: nn.le_conv(x, EI, W, t["self_kernel"], t["self_bias"], t["aggr_self_kernel"], t["aggr_self_bias"],
                                 t["aggr_neighbor_kernel"], t["aggr_neighbor_bias"], relu)),
        ("GIN", tfg.layers.GIN(mlp, train_eps=True), dict(eps=np.float32(0.3)),
         lambda x, t: nn.gin(x, EI, mlp, t["eps"])),
    ]


def test_layers_list_every_weight_and_get_the_functional_gradients(tfg):
    dev = tfg._lib.device()
    rng = np.random.Generator(np.random.PCG64(6))
    x = torch.as_tensor(_x(rng)).to(dev)
    for name, layer, ws, call in _layer_specs(tfg, rng):
        layer._maybe_build([x])
        assert sorted(layer.weights) == sorted(ws), "{}: weights {} vs {}".format(name, sorted(layer.weights), sorted(ws))
        built = {k: tuple(v.shape) for k, v in layer.weights.items()}
        layer.set_weights(**ws)
        assert {k: tuple(v.shape) for k, v in layer.weights.items()} == built, name + ": set_weights changed a weight's shape"
        layer.trainable(True)
        params = layer.parameters()
        assert len(params) == len(ws) and {id(q) for q in params} == {id(v) for v in layer.weights.values()}, name
        assert all(q.requires_grad and q.is_leaf for q in params), name
        for k in ws:      # the attribute the call reads IS the listed parameter
            assert any(getattr(layer, a, None) is layer.weights[k] for a in vars(layer)), "{}: {} is not an attribute".format(name, k)
        out = layer([x, EI, W])
        G = torch.randn(out.shape, generator=torch.Generator().manual_seed(2)).to(dev)
        out.backward(G)
        leaves = {k: torch.as_tensor(np.asarray(v, np.float32)).to(dev).requires_grad_(True) for k, v in ws.items()}
        ref = call(x, leaves)
        ref.backward(G)
        assert torch.equal(out, ref), name + ": layer output differs from the nn.* call"
        for k in ws:
            got = layer.weights[k].grad
            assert got is not None, "{}: no gradient for {}".format(name, k)
            assert float(got.abs().sum()) > 0, "{}: zero gradient for {}".format(name, k)
            assert torch.equal(got, leaves[k].grad), "{}: d/d{} differs from the nn.* call's".format(name, k)
        print("{}: {} parameters, gradients bit-identical to the functional call".format(name, len(params)))
