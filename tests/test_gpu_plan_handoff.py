# coding=utf-8
"""What the layers COMPUTE over a CSR plan that a producer handed on as ``edge_index._tfgx_plan`` (the neighbour sampler,
sag_pool, drop_edge, and chains of them), forward and backward, and what happens to an attached plan once the tensor it
describes has been written to.

One directed graph of 300 nodes / about 3600 edges: self-loops, duplicated edges, rows without in-edges, one node without any
edge, and one node whose in- and out-degree (200) are both far beyond 8x the mean, so that the forward AND the transposed
plan have a walk order (row_order) and — with plan.HUB_THRESHOLD / HUB_CHUNK forced to 32 / 16 for the module — hub lists.

For every (producer, consumer) pair:
  * bit identity: run A on the produced tensor (carries the plan), run B on ``produced.clone()`` (no attribute: CsrPlan.build
    sorts).  Output and every gradient are compared bit for bit (int32 views: max-pool GraphSAGE carries float32 lowest of
    a row without in-edges through a GEMM, which may overflow to NaN on both sides alike).
  * no second sort: CsrPlan.build is counted.  Run A's forward builds nothing and its backward at most ONE plan (the
    transposed one); behind drop_edge with a transposed parent (`*dropped_t`) the backward builds nothing either.  One
    consumer needs the transposed plan already in its forward — GCN with sym=False (column degrees) — so for it the one
    allowed build may happen in the forward; forward + backward still build at most one.  Run B builds at least one.
  * float64 anchor (bit identity alone would pass a shared wrong plan), fed the produced list as plain CPU arrays:
      - GCN, mean GraphSAGE, GAT: tests/f64_layers.py at test_gpu_backward.py's bars (test_gcn_layer_grads: forward 1e-5,
        d/dx 2e-5, weights 1e-4; test_mean_sum_sage_layer_grads_fused_epilogues and test_gat_layer_grads: forward 1e-5,
        d/dx 5e-5, weights 2e-4).  GCN sym=False has no f64_layers function: the dense float64 restatement of
        test_gcn_layer_grads (oracle.gcn_norm_adj) with the same kink rule.
      - max-pool GraphSAGE: f64_layers.max_pool_sage_layer, its default kink / tie margins, rows without in-edges excluded
        from the forward comparison as in test_pool_mlp_max_weight_gradient_from_destination_rows; the GraphSAGE bars above.
      - LSTM GraphSAGE: tests/lstm_mirror.py in float64, bar = test_gpu_lstm_sage.check (4x the error of the float32 CPU
        mirror, floor 1e-6); entries of the upstream gradient at the output ReLU's kink (|pre| <= 1e-4) are zeroed from the
        float64 forward, as f64_layers does.
      - SparseMatrix @ x: plain float64 index_add, test_aggregate_grad_x_and_w's bars (1e-5, d/dx and d/dw 2e-5).
      - edge_dot: test_gpu_linkpred's derived per-entry bounds (_check_forward, _reference_grads).
      - fused 16-bit GCN: f64_layers.gcn_layer on the widened table, test_fused_h16_layers_training's bars (1e-5, 2e-4).
    ReLU / max kinks: f64_layers' G_eff (margins 1e-4 / 2e-5) and redraw_kink_rows for GAT's Q / K projections.
Every figure is printed before it is asserted.

lstm_sage behind a pooling that keeps the hub runs T = 50 .. 110 steps over 75 .. 150 rows, almost all of them pad steps:
d/dlstm_bias sums one term per (row, pad step).  With a plain running float32 sum per lane that gradient missed
test_gpu_lstm_sage's bar (5.260e-06 against 5.229e-06 on `pooled`); tfgx_lstm_aggregate_backward_f32 now keeps a compensated
sum (1.131e-06 against the same bar)."""
import numpy as np
import pytest
import torch

import f64_layers as R
import lstm_mirror as M
from conftest import assert_parity

pytestmark = pytest.mark.gpu

N, HUB, LONE = 300, 7, 299
EMPTY_ROWS = (3, 17, 120, LONE)            # no in-edges; LONE has no out-edges either


# ---- the graph ---------------------------------------------------------------------------------------------------------
def _base_graph():
    rng = np.random.Generator(np.random.PCG64(2024))
    ei = rng.integers(0, N - 1, size=(2, 3000))
    ei = ei[:, ~np.isin(ei[0], EMPTY_ROWS)]
    loops = np.stack([np.arange(20, 40), np.arange(20, 40)])
    dups = ei[:, :200]
    hub_in = np.stack([np.full(200, HUB), rng.integers(0, N - 1, 200)])
    dst = rng.integers(0, N - 1, 200)
    dst[np.isin(dst, EMPTY_ROWS)] = HUB + 1
    hub_out = np.stack([dst, np.full(200, HUB)])
    ei = np.concatenate([ei, loops, dups, hub_in, hub_out], axis=1)
    ei = ei[:, rng.permutation(ei.shape[1])].astype(np.int32)
    w = rng.uniform(0.5, 1.5, size=ei.shape[1]).astype(np.float32)
    return ei, w


def _independent_nodes(ei, count=12):
    """Nodes (the hub excluded) that share no edge with each other and carry no self-loop."""
    nbr = [set() for _ in range(N)]
    for a, b in ei.T.tolist():
        nbr[a].add(b)
        nbr[b].add(a)
    chosen = []
    for v in range(N):
        if v != HUB and v not in nbr[v] and not any(u in nbr[v] for u in chosen):
            chosen.append(v)
            if len(chosen) == count:
                break
    assert len(chosen) == count
    return chosen


@pytest.fixture(scope="module")
def env(tfg):
    from tf_geometric_amd import plan as P
    old = P.HUB_THRESHOLD, P.HUB_CHUNK
    try:
        P.HUB_THRESHOLD, P.HUB_CHUNK = 32, 16
        ei_np, w_np = _base_graph()
        dev = tfg._lib.device()
        e = dict(ei=torch.from_numpy(ei_np).to(dev), w=torch.from_numpy(w_np).to(dev), ei_np=ei_np)
        # witnesses, before any value is compared: hub lists and a walk order on the forward and on the transposed plan
        plan = P.CsrPlan.build(e["ei"], N, N)
        for p in (plan, plan.transposed()):
            assert p.hub_info() is not None and p.row_order() is not None
            assert int(p.in_degree()[HUB]) >= 200 and int((p.in_degree() == 0).sum()) >= 1
        yield e
    finally:
        P.HUB_THRESHOLD, P.HUB_CHUNK = old


# ---- producers: stages (tfg, ei, w, n) -> (ei', w', n') ------------------------------------------------------------------
def _st_sampler(tfg, ei, w, n):
    e2, w2 = tfg.utils.RandomNeighborSampler(ei, w).sample(k=5, seed=3)
    return e2, w2, n


def _st_sampler_idx(tfg, ei, w, n):
    """Virtual ids: 199 shuffled nodes, then the node without edges — the last virtual id is never a column, so the attached
    plan is narrower than the operator the layers ask for and padded_to widens it."""
    g = torch.Generator().manual_seed(4)
    idx = torch.cat([torch.randperm(n - 1, generator=g)[:199], torch.tensor([n - 1])]).to(torch.int32).to(ei.device)
    e2, w2 = tfg.utils.RandomNeighborSampler(ei, w).sample(k=5, sampled_node_index=idx, seed=3)
    assert e2._tfgx_plan.n_src < 200 and getattr(e2._tfgx_plan, "_identity_perm", False)
    return e2, w2, 200


def _fixed_score(n, dev):
    return torch.rand(n, 1, generator=torch.Generator().manual_seed(1000 + n)).to(dev)


def _st_pooled(tfg, ei, w, n):
    dev = ei.device
    x = torch.randn(n, 4, generator=torch.Generator().manual_seed(n)).to(dev)
    score = _fixed_score(n, dev)
    if n == N:
        score[HUB] = 2.0          # the hub stays in the pooled graph
    gid = torch.zeros(n, dtype=torch.int32, device=dev)
    px, pei, pw, _ = tfg.nn.sag_pool(x, ei, w, gid, lambda inp, training=None: score, ratio=0.5)
    return pei, pw, int(px.shape[0])


def _dropped(tfg, ei, w, n, with_t, rate=0.5):
    from tf_geometric_amd import plan as P
    parent, cache = P.attached_plan(ei), None
    if parent is None:
        parent = P.CsrPlan.build(ei, n, n)
        cache = {P.CACHE_KEY_PLAN: parent}
    if with_t:
        parent.transposed()
    else:
        assert parent._transposed is None
    e2, w2 = tfg.nn.drop_edge([ei, w], rate=rate, training=True, seed=11, cache=cache)
    assert (P.attached_plan(e2)._transposed is not None) == with_t
    return e2, w2, n


def _st_dropped(tfg, ei, w, n):
    return _dropped(tfg, ei, w, n, False)


def _st_dropped_t(tfg, ei, w, n):
    return _dropped(tfg, ei, w, n, True)


def _st_dropped_all(tfg, ei, w, n):
    return _dropped(tfg, ei, w, n, True, rate=1.0)


def _st_pooled_apart(tfg, ei, w, n):
    """A pooling whose kept nodes share no edge: K = 0 edges over n_dst = 12 nodes."""
    dev = ei.device
    keep = _independent_nodes(ei.cpu().numpy())
    score = -torch.arange(n, dtype=torch.float32).reshape(n, 1)
    score[keep] += 10000.0
    score = score.to(dev)
    x = torch.randn(n, 4, generator=torch.Generator().manual_seed(n)).to(dev)
    px, pei, pw, _ = tfg.nn.sag_pool(x, ei, w, torch.zeros(n, dtype=torch.int32, device=dev),
                                     lambda inp, training=None: score, k=len(keep))
    return pei, pw, int(px.shape[0])


PRODUCERS = {
    "sampler": (_st_sampler,), "sampler_idx": (_st_sampler_idx,), "pooled": (_st_pooled,), "dropped": (_st_dropped,),
    "dropped_t": (_st_dropped_t,), "sampler>dropped_t": (_st_sampler, _st_dropped_t), "dropped>pooled": (_st_dropped, _st_pooled),
    "pooled>dropped_t": (_st_pooled, _st_dropped_t), "pooled>pooled": (_st_pooled, _st_pooled),
}
DEGENERATE = {"dropped_all": (_st_dropped_all,), "pooled_apart": (_st_pooled_apart,)}


def produce(tfg, env, name):
    from tf_geometric_amd import plan as P
    ei, w, n = env["ei"].clone(), env["w"].clone(), N
    for stage in {**PRODUCERS, **DEGENERATE}[name]:
        ei, w, n = stage(tfg, ei, w, n)
    plan = P.attached_plan(ei)
    assert plan is not None and plan.num_edges == int(ei.shape[1]) and int(w.shape[0]) == int(ei.shape[1])
    return ei, w, n


class Builds(object):
    """Counts CsrPlan.build while active."""

    def __init__(self, tfg):
        self.cls, self.n = tfg.plan.CsrPlan, 0

    def __enter__(self):
        self.real = self.cls.build

        def counted(*a, **k):
            self.n += 1
            return self.real(*a, **k)
        counted.uncounted = self.real
        self.cls.build = staticmethod(counted)
        return self

    def __exit__(self, *exc):
        self.cls.build = staticmethod(self.real)
        return False


def _fwd_bwd(builds, forward, G):
    """forward(), then the backward of (out * G).sum(); -> (out, builds in the forward, builds in the backward)."""
    b0 = builds.n
    out = forward()
    b1 = builds.n
    if out.requires_grad:
        (out * G).sum().backward()
    return out.detach(), b1 - b0, builds.n - b1


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    v = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}[a.dtype]
    assert torch.equal(a.contiguous().view(v), b.contiguous().view(v)), "{}: handed-on plan and fresh sort differ in {} elements".format(
        what, int((a.contiguous().view(v) != b.contiguous().view(v)).sum()))


def _band(what, got, ref, tol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    worst = float((np.abs(got - ref) - tol * np.abs(ref)).max()) if got.size else 0.0
    print("ANCHOR {:<60s} max(|d| - tol |ref|) = {:.3e}   bar {:.0e}".format(what, worst, tol))
    assert_parity(got, ref, tol=tol, what=what)


# ---- consumers -----------------------------------------------------------------------------------------------------------
class Consumer(object):
    """draw(n) -> state (inputs, weights, upstream gradient); anchor(state, ei, w) sets state["G"] (the upstream gradient both
    runs use) and returns a function check(tag, out, grads); run(tfg, ei_t, w_t, state, builds) -> (out, grads, fwd, bwd)."""
    name = None
    w_grad = False

    def closed_form(self, s):
        """float64 output over a list without edges (None: not compared), and the columns it covers."""
        raise NotImplementedError


def _np(t):
    return t.detach().double().cpu().numpy()


class LayerConsumer(Consumer):
    cls, f, units, kw = None, None, None, {}
    bars = None

    def weights(self, rng, oracle):
        raise NotImplementedError

    def reference(self, s, x, ei, w):
        raise NotImplementedError

    def draw(self, n, oracle):
        rng = np.random.Generator(np.random.PCG64(77 + n))
        x = torch.from_numpy(rng.standard_normal((n, self.f)).astype(np.float32))
        ws = self.weights(rng, oracle)
        G = torch.from_numpy(rng.standard_normal((n, self.units)).astype(np.float32))
        return dict(n=n, x=x, ws=ws, G=G)

    def anchor(self, s, ei, w):
        ref_out, ref, G_eff, rows = self.reference(s, ei, w)
        s["G"] = G_eff

        def check(tag, out, grads):
            _band(tag + " forward", _np(out)[rows], _np(ref_out)[rows], self.bars["out"])
            for k in ["x"] + list(s["ws"]):
                _band(tag + " d/d" + k, _np(grads[k]), _np(ref[k]), self.bars.get(k, self.bars["w"]))
        return check

    def run(self, tfg, ei_t, w_t, s, builds):
        dev = ei_t.device
        layer = getattr(tfg.layers, self.cls)(self.units, activation=tfg.relu, **self.kw)
        layer._maybe_build([s["x"]])
        layer.set_weights(**s["ws"])
        layer.trainable(True)
        xt = s["x"].to(dev).requires_grad_(True)
        out, fwd, bwd = _fwd_bwd(builds, lambda: layer([xt, ei_t, w_t], cache={}), s["G"].to(dev))
        grads = {k: layer.weights[k].grad for k in s["ws"]}
        grads["x"] = xt.grad
        return out, grads, fwd, bwd


class Gcn(LayerConsumer):
    name, cls, f, units = "gcn", "GCN", 12, 24
    bars = dict(out=1e-5, x=2e-5, w=1e-4)

    def weights(self, rng, oracle):
        return dict(kernel=oracle.glorot_uniform(rng, self.f, self.units),
                    bias=(rng.standard_normal(self.units) * 0.1).astype(np.float32))

    def reference(self, s, ei, w):
        out, g, G_eff = R.gcn_layer(s["x"], ei, w, s["ws"]["kernel"], s["ws"]["bias"], s["G"])
        return out, g, G_eff, slice(None)

    def closed_form(self, s):
        x, ws = s["x"].double().numpy(), s["ws"]
        return np.maximum(x @ ws["kernel"].astype(np.float64) + ws["bias"], 0), slice(None)


class GcnNoSym(Gcn):
    name, kw = "gcn_nosym", dict(sym=False)

    def __init__(self, oracle):
        self.oracle = oracle

    def reference(self, s, ei, w):
        n = s["n"]
        idx, nw = self.oracle.gcn_norm_adj(ei.numpy(), w.numpy(), n, sym=False)
        A = torch.zeros(n, n, dtype=torch.float64).index_put((torch.from_numpy(idx[0]).long(), torch.from_numpy(idx[1]).long()),
                                                             torch.from_numpy(nw).double(), accumulate=True)
        x = s["x"].double().requires_grad_(True)
        k = torch.from_numpy(s["ws"]["kernel"]).double().requires_grad_(True)
        b = torch.from_numpy(s["ws"]["bias"]).double().requires_grad_(True)
        out, G_eff = R._outer_relu(A @ (x @ k) + b, s["G"], 1e-4)
        out.backward(G_eff)
        return out.detach(), {"x": x.grad, "kernel": k.grad, "bias": b.grad}, G_eff.float(), slice(None)


class MeanSage(LayerConsumer):
    name, cls, f, units, kw = "mean_sage", "MeanGraphSage", 10, 32, dict(concat=True)
    bars = dict(out=1e-5, x=5e-5, w=2e-4)

    def weights(self, rng, oracle):
        ku = self.units // 2
        return dict(self_kernel=oracle.glorot_uniform(rng, self.f, ku), neighbor_kernel=oracle.glorot_uniform(rng, self.f, ku),
                    bias=(rng.standard_normal(self.units) * 0.3).astype(np.float32))

    def reference(self, s, ei, w):
        ws = s["ws"]
        out, g, G_eff = R.mean_sage_layer(s["x"], ei, w, ws["self_kernel"], ws["neighbor_kernel"], ws["bias"], s["G"])
        return out, g, G_eff, slice(None)

    def closed_form(self, s):
        x, ws, ku = s["x"].double().numpy(), s["ws"], self.units // 2
        return np.maximum(np.concatenate([x @ ws["self_kernel"].astype(np.float64), np.zeros((s["n"], ku))], 1) + ws["bias"], 0), slice(None)


class MaxPoolSage(LayerConsumer):
    name, cls, f, units, kw = "max_pool_sage", "MaxPoolGraphSage", 4, 64, dict(concat=True)
    bars = dict(out=1e-5, x=5e-5, w=2e-4)

    def weights(self, rng, oracle):
        ku = self.units // 2
        return dict(self_kernel=oracle.glorot_uniform(rng, self.f, ku), mlp_kernel=oracle.glorot_uniform(rng, self.f, 4 * ku),
                    mlp_bias=(rng.standard_normal(4 * ku) * 0.1).astype(np.float32),
                    neighs_kernel=oracle.glorot_uniform(rng, 4 * ku, ku), bias=(rng.standard_normal(self.units) * 0.1).astype(np.float32))

    def reference(self, s, ei, w):
        ws = s["ws"]
        out, g, G_eff, ambiguous = R.max_pool_sage_layer(s["x"], ei, ws["self_kernel"], ws["mlp_kernel"], ws["mlp_bias"],
                                                         ws["neighs_kernel"], ws["bias"], s["G"])
        has = (torch.bincount(ei[0].long(), minlength=s["n"]) > 0).numpy()
        assert int(ambiguous.sum()) < s["n"] // 2
        return out, g, G_eff, has

    def closed_form(self, s):      # the pooled half is float32 lowest through a GEMM: only the self half is stated
        x, ws, ku = s["x"].double().numpy(), s["ws"], self.units // 2
        return np.maximum(x @ ws["self_kernel"].astype(np.float64) + ws["bias"][:ku], 0), (slice(None), slice(0, ku))


class Gat(LayerConsumer):
    name, cls, f, units, kw = "gat", "GAT", 9, 16, dict(attention_units=8, num_heads=4)
    bars = dict(out=1e-5, x=5e-5, w=2e-4)

    def weights(self, rng, oracle):
        a, u = 8, self.units
        return dict(query_kernel=oracle.glorot_uniform(rng, self.f, a), key_kernel=oracle.glorot_uniform(rng, self.f, a),
                    kernel=oracle.glorot_uniform(rng, self.f, u), query_bias=(rng.standard_normal(a) * 0.3).astype(np.float32),
                    key_bias=(rng.standard_normal(a) * 0.3).astype(np.float32), bias=(rng.standard_normal(u) * 0.1).astype(np.float32))

    def draw(self, n, oracle):
        s = LayerConsumer.draw(self, n, oracle)
        ws = s["ws"]
        s["x"], _ = R.redraw_kink_rows(s["x"], [(ws["query_kernel"], ws["query_bias"]), (ws["key_kernel"], ws["key_bias"])])
        return s

    def reference(self, s, ei, w):
        ws = s["ws"]
        out, g, G_eff = R.gat_layer(s["x"], ei, ws["query_kernel"], ws["query_bias"], ws["key_kernel"], ws["key_bias"],
                                    ws["kernel"], ws["bias"], 4, s["G"])
        return out, g, G_eff, slice(None)

    def closed_form(self, s):      # every row attends to its self-loop alone: weight 1 / (1 + 1e-8)
        x, ws = s["x"].double().numpy(), s["ws"]
        return np.maximum(x @ ws["kernel"].astype(np.float64) / (1.0 + 1e-8) + ws["bias"], 0), slice(None)


class _LstmWeights(object):
    def __init__(self, kernel, recurrent_kernel, bias):
        self.kernel, self.recurrent_kernel, self.bias = kernel, recurrent_kernel, bias


class LstmSage(Consumer):
    """tfg.nn.lstm_graph_sage (what layers.LSTMGraphSage calls), U = 16, F = 7, T = lstm_max_degree of the list."""
    name = "lstm_sage"
    NAMES = ("x", "kernel", "recurrent_kernel", "lstm_bias", "self_kernel", "neighbor_kernel", "bias")

    def draw(self, n, oracle):
        g = torch.Generator().manual_seed(55 + n)
        U, F = 16, 7
        r = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)      # noqa: E731
        t = dict(x=r(n, F), kernel=r(F, 4 * U) / np.sqrt(F), recurrent_kernel=r(U, 4 * U) / np.sqrt(U), lstm_bias=r(4 * U) * 0.3,
                 self_kernel=r(F, U) / np.sqrt(F), neighbor_kernel=r(U, U) / np.sqrt(U), bias=r(2 * U) * 0.2)
        t = {k: v.float().double() for k, v in t.items()}        # float32-representable: all three evaluations see the same inputs
        return dict(n=n, t=t, G=r(n, 2 * U).float())

    def _mirror(self, s, ei, dtype, activation, G):
        t = {k: v.to(dtype).clone().requires_grad_(G is not None) for k, v in s["t"].items()}
        out = M.lstm_sage_mirror(t["x"], ei, t["kernel"], t["recurrent_kernel"], t["lstm_bias"], t["self_kernel"],
                                 t["neighbor_kernel"], t["bias"], activation, True, False)
        if G is None:
            return out.detach().double(), {}
        (out * G.to(dtype)).sum().backward()
        return out.detach().double(), {k: v.grad.double() for k, v in t.items()}

    def anchor(self, s, ei, w):
        from test_gpu_lstm_sage import check as lstm_check
        pre, _ = self._mirror(s, ei, torch.float64, None, None)
        s["G"] = s["G"] * (pre.abs() > 1e-4)
        ref, gref = self._mirror(s, ei, torch.float64, "relu", s["G"])
        cpu, gcpu = self._mirror(s, ei, torch.float32, "relu", s["G"])

        def check(tag, out, grads):
            lstm_check("ANCHOR " + tag + " forward", out.double().cpu(), ref, cpu)
            for k in self.NAMES:
                lstm_check("ANCHOR {} d/d{}".format(tag, k), grads[k].double().cpu(), gref[k], gcpu[k])
        return check

    def run(self, tfg, ei_t, w_t, s, builds):
        dev = ei_t.device
        t = {k: v.float().to(dev).requires_grad_(True) for k, v in s["t"].items()}
        out, fwd, bwd = _fwd_bwd(builds, lambda: tfg.nn.lstm_graph_sage(
            t["x"], ei_t, _LstmWeights(t["kernel"], t["recurrent_kernel"], t["lstm_bias"]), t["self_kernel"], t["neighbor_kernel"],
            bias=t["bias"], activation=tfg.activations.relu, cache={}), s["G"].to(dev))
        return out, {k: v.grad for k, v in t.items()}, fwd, bwd

    def closed_form(self, s):
        t = {k: v.numpy() for k, v in s["t"].items()}
        return np.maximum(np.concatenate([t["x"] @ t["self_kernel"], np.zeros((s["n"], 16))], 1) + t["bias"], 0), slice(None)


class Spmm(Consumer):
    """SparseMatrix(ei, w, [n, n]) @ x with the gradient reaching w."""
    name, w_grad = "spmm", True

    def draw(self, n, oracle):
        rng = np.random.Generator(np.random.PCG64(31 + n))
        return dict(n=n, x=torch.from_numpy(rng.standard_normal((n, 12)).astype(np.float32)),
                    G=torch.from_numpy(rng.standard_normal((n, 12)).astype(np.float32)))

    def anchor(self, s, ei, w):
        x, wr = s["x"].double().requires_grad_(True), w.double().requires_grad_(True)
        ref = torch.zeros(s["n"], 12, dtype=torch.float64).index_add(0, ei[0].long(), x[ei[1].long()] * wr[:, None])
        (ref * s["G"].double()).sum().backward()

        def check(tag, out, grads):
            _band(tag + " forward", _np(out), _np(ref), 1e-5)
            _band(tag + " d/dx", _np(grads["x"]), _np(x.grad), 2e-5)
            _band(tag + " d/dw", _np(grads["w"]), _np(wr.grad), 2e-5)
        return check

    def run(self, tfg, ei_t, w_t, s, builds):
        dev = ei_t.device
        xt, wt = s["x"].to(dev).requires_grad_(True), w_t.detach().clone().requires_grad_(True)
        n = s["n"]
        out, fwd, bwd = _fwd_bwd(builds, lambda: tfg.SparseMatrix(ei_t, wt, [n, n]) @ xt, s["G"].to(dev))
        return out, {"x": xt.grad, "w": wt.grad}, fwd, bwd

    def closed_form(self, s):
        return np.zeros((s["n"], 12)), slice(None)


class EdgeDot(Consumer):
    """edge_dot over the list, shared table, gradients recorded.  The upstream gradient is per EDGE: drawn in anchor()."""
    name = "edge_dot"
    F = 16

    def draw(self, n, oracle):
        rng = np.random.Generator(np.random.PCG64(41 + n))
        return dict(n=n, z=rng.standard_normal((n, self.F)).astype(np.float32), G=torch.zeros(0))

    def anchor(self, s, ei, w):
        from test_gpu_linkpred import _check_forward, _reference_grads
        ei_np, z = ei.numpy().astype(np.int32), s["z"]
        g = np.random.Generator(np.random.PCG64(43)).standard_normal(ei_np.shape[1]).astype(np.float32)
        s["G"] = torch.from_numpy(g)
        (ref,), (bound,) = _reference_grads(ei_np, z, z, g, True)

        def check(tag, out, grads):
            _check_forward(_np(out), z.astype(np.float64), z.astype(np.float64), ei_np, self.F, tag + " forward")
            err = np.abs(_np(grads["z"]) - ref)
            print("ANCHOR {:<60s} worst err / bound = {:.3f}   (bar 1: test_gpu_linkpred's derived bound)".format(
                tag + " d/dz", float((err / np.maximum(bound, 1e-300)).max())))
            assert (err <= bound).all(), tag + " d/dz"
        return check

    def run(self, tfg, ei_t, w_t, s, builds):
        zt = torch.from_numpy(s["z"]).to(ei_t.device).requires_grad_(True)
        out, fwd, bwd = _fwd_bwd(builds, lambda: tfg.nn.edge_dot(zt, ei_t), s["G"].to(ei_t.device))
        return out, {"z": zt.grad} if zt.grad is not None else {}, fwd, bwd

    def closed_form(self, s):
        return np.zeros((0,)), slice(None)


class FusedHalfGcn(Consumer):
    """prepare_half_features (bf16), then layers.GCN(256) on F = 100: the fused 16-bit launch with its side output
    (FUSED_H16_STATS), kernel and bias trained; the quantised table carries no gradient."""
    name = "fused_h16_gcn"
    F, units = 100, 256

    def draw(self, n, oracle):
        rng = np.random.Generator(np.random.PCG64(61 + n))
        x = torch.from_numpy(rng.standard_normal((n, self.F)).astype(np.float32)).to(torch.bfloat16).float()
        ws = dict(kernel=oracle.glorot_uniform(rng, self.F, self.units), bias=(rng.standard_normal(self.units) * 0.1).astype(np.float32))
        return dict(n=n, x=x, ws=ws, G=torch.from_numpy(rng.standard_normal((n, self.units)).astype(np.float32)))

    def anchor(self, s, ei, w):
        ref_out, ref, s["G"] = R.gcn_layer(s["x"], ei, w, s["ws"]["kernel"], s["ws"]["bias"], s["G"], x_grad=False)

        def check(tag, out, grads):
            _band(tag + " forward", _np(out), _np(ref_out), 1e-5)
            for k in s["ws"]:
                _band(tag + " d/d" + k, _np(grads[k]), _np(ref[k]), 2e-4)
        return check

    def run(self, tfg, ei_t, w_t, s, builds):
        from tf_geometric_amd import plan as P
        dev = ei_t.device
        h = tfg.prepare_half_features(s["x"].to(dev), dtype=torch.bfloat16)
        assert torch.equal(h.float().cpu(), s["x"])
        layer = tfg.layers.GCN(self.units, activation=tfg.relu)
        layer._maybe_build([s["x"]])
        layer.set_weights(**s["ws"])
        layer.trainable(True)
        before = P.FUSED_H16_STATS["launches"], P.FUSED_STATS["with_side_output"]
        out, fwd, bwd = _fwd_bwd(builds, lambda: layer([h, ei_t, w_t], cache={}), s["G"].to(dev))
        assert P.FUSED_H16_STATS["launches"] == before[0] + 1 and P.FUSED_STATS["with_side_output"] == before[1] + 1, \
            "the 16-bit GCN left its fused launch"
        return out, {k: layer.weights[k].grad for k in s["ws"]}, fwd, bwd

    def closed_form(self, s):
        x, ws = s["x"].double().numpy(), s["ws"]
        return np.maximum(x @ ws["kernel"].astype(np.float64) + ws["bias"], 0), slice(None)


CONSUMERS = ("gcn", "gcn_nosym", "mean_sage", "max_pool_sage", "gat", "lstm_sage", "spmm", "edge_dot", "fused_h16_gcn")


def consumer(name, oracle):
    return {"gcn": Gcn, "gcn_nosym": lambda: GcnNoSym(oracle), "mean_sage": MeanSage, "max_pool_sage": MaxPoolSage, "gat": Gat,
            "lstm_sage": LstmSage, "spmm": Spmm, "edge_dot": EdgeDot, "fused_h16_gcn": FusedHalfGcn}[name]()


def _run(c, tfg, ei_t, w_t, s):
    with Builds(tfg) as builds:
        return c.run(tfg, ei_t, w_t, s, builds)


# ---- part 1: every (producer, consumer) pair --------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CONSUMERS)
@pytest.mark.parametrize("pname", list(PRODUCERS))
def test_handed_on_plan(tfg, oracle, env, pname, cname):
    ei_t, w_t, n = produce(tfg, env, pname)
    c = consumer(cname, oracle)
    s = c.draw(n, oracle)
    check = c.anchor(s, ei_t.cpu(), w_t.cpu())
    tag = "{} | {}".format(pname, cname)
    out_a, g_a, fwd_a, bwd_a = _run(c, tfg, ei_t, w_t, s)
    out_b, g_b, fwd_b, bwd_b = _run(c, tfg, ei_t.clone(), w_t, s)
    print("BUILDS {}: handed-on forward {} backward {}; fresh sort forward {} backward {}".format(tag, fwd_a, bwd_a, fwd_b, bwd_b))
    # float64 first: a wrong plan is reported as wrong values, not as a mismatch between two runs
    check(tag, out_a, g_a)
    _same_bits(out_a, out_b, tag + " output")
    assert set(g_a) == set(g_b) and all(v is not None for v in g_a.values())
    for k in g_a:
        _same_bits(g_a[k], g_b[k], "{} d/d{}".format(tag, k))
    if c.w_grad:
        assert tuple(g_a["w"].shape) == (int(ei_t.shape[1]),)
    derived_t = pname.endswith("dropped_t")
    if cname == "gcn_nosym":          # column degrees: the transposed plan is needed in the forward already
        assert fwd_a <= (0 if derived_t else 1), tag
    else:
        assert fwd_a == 0, "{}: the forward sorted a list that carries its plan".format(tag)
    assert fwd_a + bwd_a <= (0 if derived_t else 1), "{}: {} + {} plans built over a handed-on plan".format(tag, fwd_a, bwd_a)
    assert fwd_b + bwd_b >= 1, tag


@pytest.mark.parametrize("cname", CONSUMERS)
@pytest.mark.parametrize("pname", list(DEGENERATE))
def test_handed_on_plan_without_edges(tfg, oracle, env, pname, cname):
    """drop_edge at rate 1.0 (K = 0 over 300 nodes) and a pooling whose 12 kept nodes share no edge: the consumer's no-edge
    result (self and bias terms; GAT: the self-loop alone, weight 1 / (1 + 1e-8)) at the forward bar 1e-5, the bits of the
    run on a clone, finite gradients, an edge-weight gradient of shape [0]."""
    ei_t, w_t, n = produce(tfg, env, pname)
    assert int(ei_t.shape[1]) == 0 and n > 0 and tuple(w_t.shape) == (0,)
    c = consumer(cname, oracle)
    s = c.draw(n, oracle)
    tag = "{} | {}".format(pname, cname)
    if cname == "max_pool_sage":
        # f64_layers.max_pool_sage_layer's rule: a row without in-edges pools float32 lowest, which overflows in the next GEMM,
        # and receives no upstream gradient — here that is every row
        s["G"] = torch.zeros_like(s["G"])
    out_a, g_a, _, _ = _run(c, tfg, ei_t, w_t, s)
    out_b, g_b, _, _ = _run(c, tfg, ei_t.clone(), w_t, s)
    ref, part = c.closed_form(s)
    _band(tag + " forward (no edges)", _np(out_a)[part], ref, 1e-5)
    _same_bits(out_a, out_b, tag + " output")
    assert set(g_a) == set(g_b)
    for k in g_a:
        # (an operand the no-edge result does not depend on — the LSTM's own weights at T = 0 — has no gradient: None)
        assert (g_a[k] is None) == (g_b[k] is None), "{} d/d{}".format(tag, k)
        if g_a[k] is not None:
            assert bool(torch.isfinite(g_a[k]).all()), "{} d/d{}".format(tag, k)
            _same_bits(g_a[k], g_b[k], "{} d/d{}".format(tag, k))
    assert cname == "edge_dot" or any(v is not None for v in g_a.values()), tag
    if c.w_grad:
        assert tuple(g_a["w"].shape) == (0,)


# ---- part 2: an attached plan whose tensor was written to, or that belongs to another list --------------------------------
def _plan_arrays_equal(a, b, what):
    assert (a.n_dst, a.n_src, a.num_edges) == (b.n_dst, b.n_src, b.num_edges), what
    for k in ("row_ptr", "col", "perm"):
        assert torch.equal(getattr(a, k), getattr(b, k)), "{}: {}".format(what, k)


def _entry_points(tfg, t, w, n):
    """What every consumer entry point makes of (t, w): plans as (row_ptr, col, perm) triples, tensors as they are."""
    from tf_geometric_amd import plan as P
    dev = t.device
    res = {}

    def arrays(plan):
        return None if plan is None else (plan.n_dst, plan.n_src, plan.row_ptr.clone(), plan.col.clone(), plan.perm.clone())

    def handed_on(ei_out, m):
        """The produced list, and its attached plan held against a sort of the list."""
        att = P.attached_plan(ei_out)
        if att is not None:
            build = getattr(P.CsrPlan.build, "uncounted", P.CsrPlan.build)
            _plan_arrays_equal(att.padded_to(m, m), build(ei_out.clone(), m, m), "derived from a stale plan")
        return ei_out.clone()

    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, 6, generator=gen).to(dev)
    gid = torch.zeros(n, dtype=torch.int32, device=dev)
    res["from_cache"] = arrays(P.CsrPlan.from_cache(t, n, n))
    adj = tfg.SparseMatrix(t, w, [n, n])
    res["sparse_plan"] = arrays(adj.plan)
    res["sparse_matmul"] = adj @ x
    d_ei, d_w = tfg.nn.drop_edge([t, w], rate=0.5, training=True, seed=5)
    res["drop_edge"], res["drop_edge_w"] = handed_on(d_ei, n), d_w
    idx = torch.randperm(n, generator=gen)[:n // 2].to(torch.int32).to(dev)
    sx, s_ei, s_w, _ = tfg.utils.sample_new_graph_by_node_index(t, idx, x=x, edge_weight=w)
    res["sample_new_graph"], res["sample_new_graph_w"] = handed_on(s_ei, n // 2), s_w
    px, p_ei, p_w, _ = tfg.nn.sort_pool(x, t, w, gid, ratio=0.5)
    res["sort_pool"], res["sort_pool_w"] = handed_on(p_ei, int(px.shape[0])), p_w
    score = _fixed_score(n, dev)
    px, p_ei, p_w, _ = tfg.nn.sag_pool(x, t, w, gid, lambda inp, training=None: score, ratio=0.5)
    res["sag_pool"], res["sag_pool_w"] = handed_on(p_ei, int(px.shape[0])), p_w
    z = torch.randn(n, 8, generator=gen).to(dev).requires_grad_(True)
    out = tfg.nn.edge_dot(z, t)
    out.backward(torch.randn(int(t.shape[1]), generator=gen).to(dev))
    res["edge_dot"], res["edge_dot_grad"] = out.detach(), z.grad
    return res


def _same_results(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], tuple):
            assert a[k][:2] == b[k][:2] and all(torch.equal(p, q) for p, q in zip(a[k][2:], b[k][2:])), "{}: {}".format(what, k)
        else:
            assert torch.equal(a[k], b[k]), "{}: {}".format(what, k)


@pytest.mark.parametrize("edit", ["shift_sources", "swap_two", "noop"])
@pytest.mark.parametrize("pname", list(PRODUCERS))
def test_attached_plan_is_dropped_after_an_in_place_write(tfg, env, pname, edit):
    """t carries a plan; t is then written to in place.  Every entry point must give what it gives for t.clone() — a plan
    equal to CsrPlan.build(t.clone()) and the same outputs (a no-op write may cost a rebuild, never a result)."""
    from tf_geometric_amd import plan as P
    t, w, n = produce(tfg, env, pname)
    old = P.attached_plan(t)
    before = t.clone()
    if edit == "shift_sources":
        t[1].add_(1).remainder_(n)
    elif edit == "swap_two":          # the sources of the first and the last edge of the list, which lie in different rows
        i, j = 0, int(t.shape[1]) - 1
        if int(t[0, i]) == int(t[0, j]) or int(t[1, i]) == int(t[1, j]):
            j = int(((t[0] != t[0, i]) & (t[1] != t[1, i])).nonzero()[0])
        a, b = int(t[1, i]), int(t[1, j])
        t[1, i], t[1, j] = b, a
    else:
        t.add_(0)
    assert torch.equal(t, before) == (edit == "noop")
    assert getattr(t, "_tfgx_plan", None) is old            # the attribute survives the write: the helper has to refuse it
    assert P.attached_plan(t) is None
    _same_results(_entry_points(tfg, t, w, n), _entry_points(tfg, t.clone(), w, n), "{} after {}".format(pname, edit))
    _plan_arrays_equal(P.CsrPlan.from_cache(t, n, n), P.CsrPlan.build(t.clone(), n, n), "from_cache after " + edit)


def test_unedited_list_keeps_its_plan(tfg, env):
    """The guard must not cost the hand-off: an untouched produced list still serves its plan at every entry point."""
    from tf_geometric_amd import plan as P
    t, w, n = produce(tfg, env, "dropped_t")
    plan = P.attached_plan(t)
    with Builds(tfg) as builds:
        assert P.CsrPlan.from_cache(t, n, n) is plan and tfg.SparseMatrix(t, w, [n, n]).plan is plan
        first = _entry_points(tfg, t, w, n)
        assert builds.n == 0, "{} plans were built for a list that carries its plan".format(builds.n)
    assert P.attached_plan(t) is plan
    _same_results(first, _entry_points(tfg, t.clone(), w, n), "unedited")


def test_widened_sampler_plan_keeps_the_identity_short_cut(tfg, env):
    """padded_to on a sampler plan: the widened plan is a new object that still knows its perm is the identity, so
    edge_attr_to_csr hands the caller's weights back without a permute launch."""
    from tf_geometric_amd import plan as P
    t, w, n = produce(tfg, env, "sampler_idx")
    att = P.attached_plan(t)
    plan = P.CsrPlan.from_cache(t, n, n)
    assert plan is not att and (plan.n_dst, plan.n_src) == (n, n) and plan.col is att.col
    assert getattr(plan, "_identity_perm", False) and plan.edge_attr_to_csr(w).data_ptr() == w.data_ptr()
    assert torch.equal(plan.perm, torch.arange(plan.num_edges, dtype=torch.int32, device=t.device))


def test_plan_of_another_list_is_ignored(tfg, env):
    """u._tfgx_plan = t._tfgx_plan with another edge count: ignored everywhere, as drop_edge's parent rule already did."""
    from tf_geometric_amd import plan as P
    t, w, n = produce(tfg, env, "pooled")
    u = t[:, :-5].clone()
    u._tfgx_plan = t._tfgx_plan
    assert P.attached_plan(u) is None and P.attached_plan(t) is not None
    _same_results(_entry_points(tfg, u, w[:-5], n), _entry_points(tfg, u.clone(), w[:-5], n), "foreign plan")


def test_sag_pool_alias_still_hands_the_parent_plan_to_the_score_gnn(tfg, env):
    """sag_pool on a plain list: ONE plan is built; the score GNN finds it on the alias (same storage, same version counter),
    and the caller's tensor object is left without an attachment."""
    dev = env["ei"].device
    ei, w = env["ei"].clone(), env["w"]
    x = torch.randn(N, 6, generator=torch.Generator().manual_seed(2)).to(dev)
    gnn = tfg.layers.GCN(1)
    gnn._maybe_build([x])
    seen = []

    def score_gnn(inputs, training=None):
        seen.append(inputs[1])
        return gnn(inputs, training=training)
    with Builds(tfg) as builds:
        px, pei, pw, _ = tfg.nn.sag_pool(x, ei, w, torch.zeros(N, dtype=torch.int32, device=dev), score_gnn, ratio=0.5)
    assert builds.n == 1, "sag_pool built {} plans".format(builds.n)
    assert seen[0] is not ei and seen[0].data_ptr() == ei.data_ptr() and tfg.plan.attached_plan(seen[0]) is not None
    assert getattr(ei, "_tfgx_plan", None) is None
    m = int(px.shape[0])
    _plan_arrays_equal(tfg.plan.attached_plan(pei), tfg.plan.CsrPlan.build(pei.clone(), m, m), "pooled plan")
    # a write through the caller's tensor reaches the alias: its plan is refused from then on
    ei[1].add_(1).remainder_(N)
    assert tfg.plan.attached_plan(seen[0]) is None
