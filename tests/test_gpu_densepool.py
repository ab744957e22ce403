# coding=utf-8
"""DiffPool and MinCutPool on the GPU (tf_geometric_amd.nn.pool.diff_pool / min_cut_pool, layers.DiffPool / MinCutPool).

Values: the reference's own outputs (tests/golden/densepool_cases.npz): index arrays exactly, values within assert_parity's
1e-5 + 1e-5 |ref|, the two losses within 1e-5 (1 + |ref|).
Gradients: float64 autograd on the mirror (tests/densepool_mirror.py), per element max(1e-5 (1 + |ref|), 8 * 2^-24 * sqrt(k) *
sum|terms|), the bar of tests/test_gpu_fuzz_backward.py, with sum|terms| from the mirror's absolute mode and k = the number of
nodes of the batch: the weight and bias gradients sum over the nodes, and every other reduction of these gradients (over the
units, the clusters, a neighbourhood, a graph) is shorter.
Then the hand-off of the pooled list's plan, the refusals and the host reads of a warm call."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_parity
import densepool_cases as dc
import densepool_mirror as dm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "densepool_cases.npz")
EPS = 8.0 * 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def produced(tfg):
    """Every configuration of the case table, run once."""
    case = dc.CASES[0]
    return case.hip(tfg, case.inputs())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("cfg", dc.ALL_CONFIGS)
def test_outputs_against_the_reference(cfg, produced, golden):
    pre = cfg + "/"
    for name in ("edge_index", "node_graph_index"):
        got, ref = produced[pre + name], golden["densepool::" + pre + name]
        assert got.dtype == np.int32 and np.array_equal(got, ref), pre + name
    assert produced[pre + "edge_weight"].dtype == np.float32
    assert_parity(produced[pre + "x"], golden["densepool::" + pre + "x"], what=pre + "x")
    assert_parity(produced[pre + "edge_weight"], golden["densepool::" + pre + "edge_weight"], what=pre + "edge_weight")


@pytest.mark.parametrize("cfg", dc.LOSS_CONFIGS)
def test_losses_against_the_reference(cfg, produced, golden):
    for name in ("cut_loss", "orth_loss"):
        got, ref = float(produced["{}/{}".format(cfg, name)]), float(golden["densepool::{}/{}".format(cfg, name)])
        print("{}/{}: {:.7f} vs reference {:.7f}".format(cfg, name, got, ref))
        assert abs(got - ref) <= 1e-5 * (1.0 + abs(ref)), (cfg, name, got, ref)


# ---- gradients -----------------------------------------------------------------------------------------------------------
def _layers(tfg, g, kind, ignore_weights=False, **kw):
    feature, assign = dc.hip_gcn(tfg, g, "feature"), dc.hip_gcn(tfg, g, "assign")
    if ignore_weights:        # a GCN on the unweighted graph: the normalisation of a GCN takes no tracked edge_weight
        wrap = lambda layer: (lambda inputs, training=None, cache=None: layer([inputs[0], inputs[1]], training=training))  # noqa: E731
        f, a = wrap(feature), wrap(assign)
    else:
        f, a = feature, assign
    cls = tfg.layers.DiffPool if kind == "diff" else tfg.layers.MinCutPool
    layer = cls(f, a, dc.UNITS, dc.K, **kw)
    layer.set_weights(bias=g["bias"])
    return layer, feature, assign


def _compare(got, ref, absref, k):
    for name in ref:
        a, r, ar = got[name].double().cpu().numpy(), ref[name], absref[name]
        assert a.shape == r.shape and np.isfinite(a).all(), name
        bound = np.maximum(1e-5 * (1.0 + np.abs(r)), EPS * np.sqrt(k) * ar)
        err = np.abs(a - r)
        print("d/d{}: max |ref| {:.3e}, max err {:.3e}, max err / bound {:.3f}".format(
            name, float(np.abs(r).max()), float(err.max()), float((err / bound).max())))
        assert (err <= bound).all(), "d/d{}: max err / bound = {:.3f}".format(name, float((err / bound).max()))
        assert np.abs(r).max() > 1e-3, name + ": the reference gradient is trivially small"


def test_diff_pool_gradients(tfg):
    """d/d(x, the two GNNs' weights, the bias, edge_weight) of a scalar of pooled_x and pooled_edge_weight.  The GNNs are
    GCNs on the unweighted graph, so that edge_weight reaches the loss through the coarsening alone."""
    g = dc.batch()
    rng = np.random.Generator(np.random.PCG64(41))
    layer, feature, assign = _layers(tfg, g, "diff", ignore_weights=True)
    layer.trainable(True)
    feature.trainable(True)
    assign.trainable(True)
    x, w = _dev(g["x"]).requires_grad_(True), _dev(g["w"]).requires_grad_(True)
    px, pei, pw, pgi = layer([x, _dev(g["ei"]), w, _dev(g["gid"])], num_graphs=len(dc.SIZES))
    cx, cw = rng.standard_normal(tuple(px.shape)), rng.standard_normal(tuple(pw.shape))
    ((px.double() * _dev(cx)).sum() + (pw.double() * _dev(cw)).sum()).backward()
    got = dict(x=x.grad, w=w.grad, bias=layer.bias.grad, feature_kernel=feature.kernel.grad, feature_bias=feature.bias.grad,
               assign_kernel=assign.kernel.grad, assign_bias=assign.bias.grad)
    assert all(v is not None for v in got.values())

    def mirror(absolute):
        leaf = {k: torch.from_numpy(g[k]).double().requires_grad_(True) for k in
                ("x", "w", "bias", "feature_kernel", "feature_bias", "assign_kernel", "assign_bias")}

        def unweighted(which):
            return lambda ops, xx, row, col, wv: dm.gcn_mirror(ops, xx, row, col, torch.ones_like(wv).detach(),
                                                              leaf[which + "_kernel"], leaf[which + "_bias"])
        m = dm.diff_pool_mirror(leaf["x"], g["ei"], leaf["w"], g["gid"], unweighted("feature"), unweighted("assign"),
                                bias=leaf["bias"], absolute=absolute)
        assert np.array_equal(m["edge_index"], pei.cpu().numpy())
        tx, tw = torch.from_numpy(cx), torch.from_numpy(cw)
        ((m["x"] * (tx.abs() if absolute else tx)).sum() + (m["edge_weight"] * (tw.abs() if absolute else tw)).sum()).backward()
        return {k: v.grad.numpy() for k, v in leaf.items()}
    _compare(got, mirror(False), mirror(True), g["n"])


@pytest.mark.parametrize("normed", [True, False])
def test_min_cut_pool_gradients(tfg, normed):
    """d/d(x, the two GNNs' weights, the bias) of a scalar of pooled_x, pooled_edge_weight and both losses."""
    g = dc.batch()
    rng = np.random.Generator(np.random.PCG64(43))
    layer, feature, assign = _layers(tfg, g, "min_cut", gnn_use_normed_edge=normed)
    layer.trainable(True)
    assert feature.kernel.requires_grad and assign.bias.requires_grad and layer.bias.requires_grad
    assert len(layer.parameters()) == 5
    x = _dev(g["x"]).requires_grad_(True)
    (px, pei, pw, pgi), (cut, orth) = layer([x, _dev(g["ei"]), _dev(g["w"]), _dev(g["gid"])], return_losses=True)
    cx, cw = rng.standard_normal(tuple(px.shape)), rng.standard_normal(tuple(pw.shape))
    ((px.double() * _dev(cx)).sum() + (pw.double() * _dev(cw)).sum() + 3.0 * cut.double() + 2.0 * orth.double()).backward()
    got = dict(x=x.grad, bias=layer.bias.grad, feature_kernel=feature.kernel.grad, feature_bias=feature.bias.grad,
               assign_kernel=assign.kernel.grad, assign_bias=assign.bias.grad)
    assert all(v is not None for v in got.values())
    both = layer.losses          # the callable of the latest call, after the (absent) regulariser terms
    assert len(both) == 2 and torch.equal(both[0], cut) and torch.equal(both[1], orth)

    def mirror(absolute):
        leaf = {k: torch.from_numpy(g[k]).double().requires_grad_(True) for k in
                ("x", "bias", "feature_kernel", "feature_bias", "assign_kernel", "assign_bias")}
        m = dm.min_cut_pool_mirror(leaf["x"], g["ei"], g["w"], g["gid"], (leaf["feature_kernel"], leaf["feature_bias"]),
                                   (leaf["assign_kernel"], leaf["assign_bias"]), bias=leaf["bias"], gnn_use_normed_edge=normed,
                                   absolute=absolute)
        assert np.array_equal(m["edge_index"], pei.cpu().numpy())
        tx, tw = torch.from_numpy(cx), torch.from_numpy(cw)
        ((m["x"] * (tx.abs() if absolute else tx)).sum() + (m["edge_weight"] * (tw.abs() if absolute else tw)).sum()
         + 3.0 * m["cut_loss"] + 2.0 * m["orth_loss"]).backward()
        return {k: v.grad.numpy() for k, v in leaf.items()}
    _compare(got, mirror(False), mirror(True), g["n"])


def test_loss_gradient_with_respect_to_the_assignment(tfg):
    g = dc.batch()
    S = _dev(g["assign"]).requires_grad_(True)
    cut, orth = tfg.nn.min_cut_pool_compute_losses(_dev(g["ei"]), _dev(g["w"]), _dev(g["gid"]), S)
    (3.0 * cut.double() + 2.0 * orth.double()).backward()

    def mirror(absolute):
        leaf = torch.from_numpy(g["assign"]).double().requires_grad_(True)
        c, o = dm.min_cut_losses_mirror(g["ei"], g["w"], g["gid"], leaf, absolute=absolute)
        (3.0 * c + 2.0 * o).backward()
        return dict(assign=leaf.grad.numpy())
    _compare(dict(assign=S.grad), mirror(False), mirror(True), g["n"])


# ---- hand-off ------------------------------------------------------------------------------------------------------------
class Builds(object):
    """Counts CsrPlan.build while active."""

    def __init__(self, tfg):
        self.cls, self.n = tfg.plan.CsrPlan, 0

    def __enter__(self):
        self.real = self.cls.build

        def counted(*a, **k):
            self.n += 1
            return self.real(*a, **k)
        self.cls.build = staticmethod(counted)
        return self

    def __exit__(self, *exc):
        self.cls.build = staticmethod(self.real)
        return False


@pytest.mark.parametrize("fn", ["diff_pool_coarsen", "min_cut_pool_coarsen"])
def test_the_attached_plan_is_the_built_plan(tfg, fn):
    from tf_geometric_amd.plan import CsrPlan, attached_plan
    g = dc.batch()
    px, pei, pw, pgi = getattr(tfg.nn, fn)(_dev(g["x"]), _dev(g["ei"]), _dev(g["w"]), _dev(g["gid"]), _dev(g["assign"]))
    assert isinstance(pei, torch.Tensor) and pei.dtype == torch.int32 and pgi.dtype == torch.int32
    n = len(dc.SIZES) * dc.K
    handed, built = attached_plan(pei), CsrPlan.build(pei.clone(), n, n)
    assert handed is not None and pei.shape[1] > 0
    assert (handed.n_dst, handed.n_src, handed.num_edges) == (built.n_dst, built.n_src, built.num_edges)
    for k in ("row_ptr", "col", "perm"):
        a, b = getattr(handed, k), getattr(built, k)
        assert a.dtype == b.dtype and torch.equal(a, b), k


def test_a_second_layer_runs_on_the_handed_on_plan(tfg):
    g = dc.batch()
    first, _, _ = _layers(tfg, g, "diff")
    px, pei, pw, pgi = first([_dev(g["x"]), _dev(g["ei"]), _dev(g["w"]), _dev(g["gid"])])

    def second(edge_index):
        f, a = tfg.layers.GCN(4, seed=1), tfg.layers.GCN(2, seed=2)
        layer = tfg.layers.DiffPool(f, a, 4, 2, seed=3)
        with Builds(tfg) as builds:
            out = layer([px, edge_index, pw, pgi], num_graphs=len(dc.SIZES))
        return out, builds.n
    out_a, builds_a = second(pei)
    out_b, builds_b = second(pei.clone())
    print("BUILDS second DiffPool layer: handed-on {} / fresh list {}".format(builds_a, builds_b))
    assert builds_a == 1, "only the CSR over graphs is built; the edge list carries its plan"
    assert builds_b > builds_a
    for a, b in zip(out_a, out_b):
        assert torch.equal(a, b)
    assert out_a[0].shape == (len(dc.SIZES) * 2, 4) and torch.isfinite(out_a[0]).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(tfg):
    g = dc.batch()
    x, ei, w, gid, S = _dev(g["x"]), _dev(g["ei"]), _dev(g["w"]), _dev(g["gid"]), _dev(g["assign"])
    a, b = int(np.flatnonzero(g["gid"] == 0)[0]), int(np.flatnonzero(g["gid"] == 3)[0])
    cross = torch.cat([ei, torch.tensor([[a], [b]], dtype=torch.int32, device=ei.device)], dim=1)
    with pytest.raises(ValueError, match="between two graphs"):
        tfg.nn.diff_pool_coarsen(x, cross, None, gid, S)
    with pytest.raises(ValueError, match="between two graphs"):
        tfg.nn.min_cut_pool_compute_losses(cross, None, gid, S)
    wide = torch.full((g["n"], 65), 1.0 / 65, device=x.device)
    with pytest.raises(ValueError, match="TFGX_SEGGRAM_MAX_K = 64"):
        tfg.nn.diff_pool_coarsen(x, ei, w, gid, wide)
    with pytest.raises(ValueError, match="TFGX_SEGGRAM_MAX_K = 64"):
        tfg.nn.min_cut_pool_coarsen(x, ei, w, gid, wide)
    layer, _, _ = _layers(tfg, g, "min_cut")
    tracked = w.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="edge_weight that requires grad"):
        layer([x, ei, tracked, gid])
    with pytest.raises(NotImplementedError, match="edge_weight that requires grad"):
        tfg.nn.min_cut_pool_compute_losses(ei, tracked, gid, S)
    with pytest.raises(ValueError, match="same time"):
        layer([x, ei, w, gid], return_loss_func=True, return_losses=True)
    # cluster_pool is untouched: it still refuses a tracked assignment weight
    assign = np.stack([np.arange(g["n"]), g["gid"]]).astype(np.int32)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        tfg.nn.cluster_pool(x, ei, w, _dev(assign), torch.ones(g["n"], device=x.device, requires_grad=True), len(dc.SIZES))


def test_refused_inside_graph_capture(tfg):
    g = dc.batch()
    args = [_dev(g["x"]), _dev(g["ei"]), _dev(g["w"]), _dev(g["gid"]), _dev(g["assign"])]
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with pytest.raises(RuntimeError, match="capture"):
            with torch.cuda.graph(graph, stream=side):
                tfg.nn.diff_pool_coarsen(*args)
    torch.cuda.synchronize()


# ---- host reads --------------------------------------------------------------------------------------------------------------
class HostReads(object):
    """Counts what brings a device value to the host while active: Tensor.item / tolist / cpu / numpy / __bool__ / __int__ /
    __float__, torch.nonzero (its result's size is data) and CsrPlan.build (the builder reports bad indices to the host)."""
    METHODS = ("item", "tolist", "cpu", "numpy", "__bool__", "__int__", "__float__", "nonzero")

    def __init__(self, tfg):
        self.plan_cls, self.seen = tfg.plan.CsrPlan, []

    def _wrap(self, name, real):
        def counted(*a, **k):
            t = a[0] if a else None
            if not isinstance(t, torch.Tensor) or t.is_cuda:
                self.seen.append(name)
            return real(*a, **k)
        return counted

    def __enter__(self):
        self.real = {m: getattr(torch.Tensor, m) for m in self.METHODS}
        for m, real in self.real.items():
            setattr(torch.Tensor, m, self._wrap(m, real))
        self.real_nonzero, self.real_build = torch.nonzero, self.plan_cls.build
        torch.nonzero = self._wrap("torch.nonzero", torch.nonzero)
        self.plan_cls.build = staticmethod(self._wrap("CsrPlan.build", self.real_build))
        return self

    def __exit__(self, *exc):
        for m, real in self.real.items():
            setattr(torch.Tensor, m, real)
        torch.nonzero = self.real_nonzero
        self.plan_cls.build = staticmethod(self.real_build)
        return False


@pytest.mark.parametrize("kind", ["diff", "min_cut"])
def test_a_warm_call_reads_the_host_once(tfg, kind):
    """With a warm cache and num_graphs given: one host read, the count of non-zero pooled entries."""
    g = dc.batch()
    layer, _, _ = _layers(tfg, g, kind)
    inputs = [_dev(g["x"]), _dev(g["ei"]), _dev(g["w"]), _dev(g["gid"])]
    cache = {}
    cold = layer(inputs, cache=cache, num_graphs=len(dc.SIZES))
    with HostReads(tfg) as reads:
        warm = layer(inputs, cache=cache, num_graphs=len(dc.SIZES))
    print("host reads of a warm {} call: {}".format(kind, reads.seen))
    assert reads.seen == ["torch.nonzero"], reads.seen
    for a, b in zip(cold, warm):
        assert torch.equal(a, b)
    with HostReads(tfg) as reads:
        layer(inputs, num_graphs=len(dc.SIZES))
    assert reads.seen.count("CsrPlan.build") >= 2 and "item" in reads.seen        # without a cache: the plans and the verdict
