# coding=utf-8
"""The GCN normalisation is differentiable in the edge weights (nn/conv/gcn.py gcn_norm_adj on tfgx_gcn_norm_backward_f32,
include/tfgx_normgrad.h), on the GPU.

Reference: float64 torch autograd on the restatement with the masked power (tests/normgrad_mirror.py).  Error bar per element:
max(1e-5 (1 + |ref|), 8 * 2^-24 * sqrt(k) * sum|terms|) — the bar of tests/test_gpu_densepool.py and test_gpu_fuzz_backward.py —
with sum|terms| from the restatement's absolute mode and k the longest reduction of the case (the largest number of edges of
one row or one column, plus 2; for layers also the node count, which the weight gradients sum over)."""
import numpy as np
import pytest
import torch

import densepool_cases as dc
import densepool_mirror as dm
import normgrad_mirror as nm
from asap_mirror import _Ops

pytestmark = pytest.mark.gpu

EPS = 8.0 * 2.0 ** -24
DEFAULT = ("both", True, True, True, False)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _check(name, got, ref, terms, k):
    a = got.detach().double().cpu().numpy()
    assert a.shape == ref.shape and np.isfinite(a).all(), name
    bound = np.maximum(1e-5 * (1.0 + np.abs(ref)), EPS * np.sqrt(k) * terms)
    err = np.abs(a - ref)
    print("d/d{}: max |ref| {:.3e}, max err {:.3e}, max err / bound {:.3f}".format(
        name, float(np.abs(ref).max()), float(err.max()), float((err / bound).max())))
    assert (err <= bound).all(), "d/d{}: max err / bound = {:.3f}".format(name, float((err / bound).max()))


def _normed(g, cfg, n_rows, n_cols, w):
    from tf_geometric_amd.nn.conv.gcn import gcn_norm_adj
    from tf_geometric_amd.sparse import SparseMatrix
    norm, sym, asl, renorm, improved = cfg
    adj = SparseMatrix(_dev(np.stack([g["row"], g["col"]])), w, [n_rows, n_cols])
    return gcn_norm_adj(adj, norm=norm, add_self_loop=asl, sym=sym, renorm=renorm, improved=improved)


def _operator_gradient(g, cfg, n_rows, n_cols, c=None):
    """d/d(value, caller's edge order) of sum_e c_e w'_e + sum_v s_v self_coef[v]."""
    w = _dev(g["w"]).requires_grad_(True)
    normed = _normed(g, cfg, n_rows, n_cols, w)
    c = g["c"] if c is None else c
    loss = (normed.w_csr.double() * _dev(c)[normed.plan.perm.long()]).sum()
    if normed.self_coef is not None:
        loss = loss + (normed.self_coef.double() * _dev(g["s"])).sum()
    loss.backward()
    return w.grad


def _against_float64(g, cfg, n_rows, n_cols):
    got = _operator_gradient(g, cfg, n_rows, n_cols)
    assert got is not None, "edge weights that require grad got no gradient through gcn_norm_adj"
    ref = nm.reference_gradient(g["row"], g["col"], g["w"], n_rows, n_cols, cfg, g["c"], g["s"])
    terms = nm.reference_gradient(g["row"], g["col"], g["w"], n_rows, n_cols, cfg, g["c"], g["s"], absolute=True)
    _check("value[{}]".format(nm.config_id(cfg)), got, ref, terms, nm.longest_reduction(g["row"], g["col"], n_rows, n_cols))
    assert np.abs(ref).max() > 1e-3
    return got


# ---- 1. operator sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", nm.configs(), ids=nm.config_id)
def test_operator_sweep(tfg, cfg):
    g = nm.sweep_graph()
    _against_float64(g, cfg, g["n"], g["n"])


def test_forward_values_are_those_of_the_untracked_route(tfg):
    g = nm.sweep_graph()
    for cfg in nm.configs():
        plain = _normed(g, cfg, g["n"], g["n"], _dev(g["w"]))
        tracked = _normed(g, cfg, g["n"], g["n"], _dev(g["w"]).requires_grad_(True))
        assert tracked.w_csr.requires_grad and not plain.w_csr.requires_grad
        assert torch.equal(plain.w_csr, tracked.w_csr.detach()), cfg
        assert (plain.self_coef is None) == (tracked.self_coef is None)
        if plain.self_coef is not None:
            assert torch.equal(plain.self_coef, tracked.self_coef.detach()), cfg


# ---- 2. zeroed factors ---------------------------------------------------------------------------------------------------------
NO_LOOP = [("both", True, False, True, False), ("both", False, False, True, False), ("left", True, False, True, False),
           ("right", True, False, True, False)]


@pytest.mark.parametrize("cfg", NO_LOOP, ids=nm.config_id)
def test_zeroed_factors_have_zero_derivative(tfg, cfg):
    """Row 2 has a negative degree, node 36 degree 0: every gradient is finite and the masked restatement's."""
    g = nm.sweep_graph(negate_row=2)
    deg = np.bincount(g["row"], weights=g["w"].astype(np.float64), minlength=g["n"])
    assert deg[36] == 0.0 and deg[2] < 0.0 and (g["col"] == 36).any()
    got = _against_float64(g, cfg, g["n"], g["n"])
    assert torch.isfinite(got).all()


def test_a_zero_degree_node_contributes_exactly_zero(tfg):
    """Cotangents on the edges into node 36 alone: their normalised weights are w p(deg[r]) p(0) = 0 whatever w is, so every
    gradient entry is exactly 0 (tf.where would have made them NaN)."""
    g = nm.sweep_graph(negate_row=2)
    c = np.where(g["col"] == 36, g["c"], 0.0)
    for cfg in (NO_LOOP[0], NO_LOOP[3]):
        got = _operator_gradient(g, cfg, g["n"], g["n"], c=c)
        assert torch.equal(got, torch.zeros_like(got)), cfg


# ---- 3. hubs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [("both", True, True, True, False), ("both", False, True, True, False),
                                 ("right", True, True, True, False)], ids=nm.config_id)
def test_hub_rows_and_hub_columns(tfg, cfg):
    g = nm.hub_graph()
    assert np.bincount(g["row"]).max() > 2048 and np.bincount(g["col"]).max() > 2048       # kLongRow
    first = _against_float64(g, cfg, g["n"], g["n"])
    second = _operator_gradient(g, cfg, g["n"], g["n"])
    assert torch.equal(first, second), "two runs differ"


# ---- 4. rectangular --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, cfg", [((7, 11), ("both", False, False, True, False)), ((7, 11), ("left", False, False, True, False)),
                                        ((11, 7), ("right", False, False, True, False))], ids=["both-7x11", "left-7x11", "right-11x7"])
def test_rectangular_operators(tfg, shape, cfg):
    _against_float64(nm.rect_graph(*shape), cfg, shape[0], shape[1])


# ---- 5. layer --------------------------------------------------------------------------------------------------------------------
F = 12


def _layer_case(units):
    g = nm.sweep_graph()
    rng = np.random.Generator(np.random.PCG64(100 + (units or 0)))
    out_w = units if units is not None else F
    g.update(x=rng.uniform(-1, 1, (g["n"], F)).astype(np.float32),
             kernel=None if units is None else (rng.uniform(-1, 1, (F, units)) * np.sqrt(6.0 / (F + units))).astype(np.float32),
             bias=rng.uniform(-0.3, 0.3, out_w).astype(np.float32), C=rng.standard_normal((g["n"], out_w)))
    return g


def _layer_forward(tfg, g, units, leaves, cache=None):
    ei = _dev(np.stack([g["row"], g["col"]]))
    if units is None:
        from tf_geometric_amd.sparse import SparseMatrix
        return tfg.nn.gcn(leaves["x"], SparseMatrix(ei, leaves["w"], [g["n"], g["n"]]), None, leaves["bias"], cache=cache)
    layer = tfg.layers.GCN(units)
    layer._maybe_build([g["x"]])
    layer.kernel, layer.bias = leaves["kernel"], leaves["bias"]
    return layer([leaves["x"], ei, leaves["w"]], cache=cache)


def _layer_reference(g, absolute):
    ops = _Ops(absolute)
    names = [k for k in ("x", "w", "kernel", "bias") if g[k] is not None]
    leaf = {k: torch.from_numpy(np.asarray(g[k], np.float64)).requires_grad_(True) for k in names}
    row, col = torch.from_numpy(g["row"].astype(np.int64)), torch.from_numpy(g["col"].astype(np.int64))
    out = nm.gcn_mirror(ops, leaf["x"], row, col, leaf["w"], g["n"], DEFAULT, leaf.get("kernel"), leaf["bias"])
    C = torch.from_numpy(g["C"])
    (out * (C.abs() if absolute else C)).sum().backward()
    return {k: v.grad.numpy() for k, v in leaf.items()}


@pytest.mark.parametrize("units", [5, 20, None], ids=["units5", "units20", "no-kernel"])
def test_layer_gradients(tfg, units):
    g = _layer_case(units)
    names = [k for k in ("x", "w", "kernel", "bias") if g[k] is not None]
    k = max(nm.longest_reduction(g["row"], g["col"], g["n"], g["n"]), g["n"] + 2, F + 2)
    ref, terms = _layer_reference(g, False), _layer_reference(g, True)

    leaves = {n: _dev(g[n]).requires_grad_(True) for n in names}
    out = _layer_forward(tfg, g, units, leaves)
    (out.double() * _dev(g["C"])).sum().backward()
    assert leaves["w"].grad is not None, "edge_weight got no gradient through the GCN"
    for n in names:
        _check("{}[{}]".format(n, units), leaves[n].grad, ref[n], terms[n], k)

    # the same values with the weight detached (x, kernel and bias still tracked: the same route)
    frozen = dict(leaves, w=leaves["w"].detach())
    assert torch.equal(out.detach(), _layer_forward(tfg, g, units, frozen).detach())

    # only edge_weight tracked: x and the kernel are frozen, the differentiable route is still taken
    only = {n: _dev(g[n]) for n in names}
    only["w"].requires_grad_(True)
    out2 = _layer_forward(tfg, g, units, only)
    assert out2.requires_grad
    (out2.double() * _dev(g["C"])).sum().backward()
    _check("w-alone[{}]".format(units), only["w"].grad, ref["w"], terms["w"], k)


# ---- 6. cache --------------------------------------------------------------------------------------------------------------------
def _stale_keys(cache):
    return [key for key in cache if str(key).startswith("gcn_normed_adj_") or key == "tfgx_gcn_adj"]


def test_a_tracked_weight_stays_out_of_the_cache(tfg):
    from tf_geometric_amd.plan import CACHE_KEY_PLAN
    g = _layer_case(5)
    leaves = {n: _dev(g[n]) for n in ("x", "w", "kernel", "bias")}
    leaves["w"].requires_grad_(True)
    cache = {}
    first = _layer_forward(tfg, g, 5, leaves, cache=cache)
    assert cache.get(CACHE_KEY_PLAN) is not None and _stale_keys(cache) == [], list(cache)
    plan = cache[CACHE_KEY_PLAN]
    doubled = dict(leaves, w=(leaves["w"].detach() * 2.0 + 0.25).requires_grad_(True))
    second = _layer_forward(tfg, g, 5, doubled, cache=cache)
    assert cache[CACHE_KEY_PLAN] is plan and _stale_keys(cache) == []
    assert torch.equal(second, _layer_forward(tfg, g, 5, doubled)) and not torch.equal(first, second)
    # an untracked weight, and a tracked one under no_grad: the keys of before
    for w in (leaves["w"].detach(), leaves["w"]):
        cache = {}
        with torch.no_grad():
            _layer_forward(tfg, g, 5, dict(leaves, w=w), cache=cache)
        assert sorted(_stale_keys(cache)) == ["gcn_normed_adj_both_True_True_True_False", "tfgx_gcn_adj"], list(cache)
    cache = {}
    _layer_forward(tfg, g, 5, dict(leaves, w=leaves["w"].detach()), cache=cache)
    assert sorted(_stale_keys(cache)) == ["gcn_normed_adj_both_True_True_True_False", "tfgx_gcn_adj"]


# ---- 7. hierarchy ----------------------------------------------------------------------------------------------------------------
def test_diff_pool_trains_through_the_next_level(tfg):
    """layers.DiffPool with its GCNs on the WEIGHTED graph, then nn.gcn on the pooled graph with the tracked pooled weights:
    d/d(x, w, both GNNs' weights, the bias, the second level's kernel) against float64."""
    from tf_geometric_amd.sparse import SparseMatrix
    g = dc.batch()
    rng = np.random.Generator(np.random.PCG64(47))
    G = len(dc.SIZES)
    g["kernel2"] = (rng.uniform(-1, 1, (dc.UNITS, 4)) * 0.7).astype(np.float32)
    names = ("x", "w", "bias", "feature_kernel", "feature_bias", "assign_kernel", "assign_bias", "kernel2")
    feature, assign = dc.hip_gcn(tfg, g, "feature"), dc.hip_gcn(tfg, g, "assign")
    layer = tfg.layers.DiffPool(feature, assign, dc.UNITS, dc.K)
    layer.set_weights(bias=g["bias"])
    for m in (layer, feature, assign):
        m.trainable(True)
    x, w, k2 = (_dev(g[n]).requires_grad_(True) for n in ("x", "w", "kernel2"))
    px, pei, pw, pgi = layer([x, _dev(g["ei"]), w, _dev(g["gid"])], num_graphs=G)
    assert pw.requires_grad
    out = tfg.nn.gcn(px, SparseMatrix(pei, pw, [G * dc.K, G * dc.K]), k2)
    C = rng.standard_normal(tuple(out.shape))
    (out.double() * _dev(C)).sum().backward()
    got = dict(x=x.grad, w=w.grad, bias=layer.bias.grad, feature_kernel=feature.kernel.grad, feature_bias=feature.bias.grad,
               assign_kernel=assign.kernel.grad, assign_bias=assign.bias.grad, kernel2=k2.grad)
    assert all(v is not None for v in got.values()), [n for n, v in got.items() if v is None]

    def mirror(absolute):
        leaf = {n: torch.from_numpy(g[n]).double().requires_grad_(True) for n in names}

        def weighted(which):
            if absolute:       # the same values, every local Jacobian absolute
                return lambda ops, xx, row, col, wv: nm.gcn_mirror(ops, xx, row, col, wv, int(xx.shape[0]), DEFAULT,
                                                                   leaf[which + "_kernel"], leaf[which + "_bias"])
            return lambda ops, xx, row, col, wv: dm.gcn_mirror(ops, xx, row, col, wv, leaf[which + "_kernel"],
                                                               leaf[which + "_bias"])
        m = dm.diff_pool_mirror(leaf["x"], g["ei"], leaf["w"], g["gid"], weighted("feature"), weighted("assign"),
                                bias=leaf["bias"], absolute=absolute)
        assert np.array_equal(m["edge_index"], pei.cpu().numpy())
        prow, pcol = (torch.from_numpy(m["edge_index"][i].astype(np.int64)) for i in (0, 1))
        ops = _Ops(absolute)
        if absolute:
            o = nm.gcn_mirror(ops, m["x"], prow, pcol, m["edge_weight"], G * dc.K, DEFAULT, leaf["kernel2"])
        else:
            o = dm.gcn_mirror(ops, m["x"], prow, pcol, m["edge_weight"], leaf["kernel2"], None)
        tc = torch.from_numpy(C)
        (o * (tc.abs() if absolute else tc)).sum().backward()
        return {n: v.grad.numpy() for n, v in leaf.items()}, o.detach().numpy()
    (ref, out_ref), (terms, out_abs) = mirror(False), mirror(True)
    assert np.allclose(out_ref, out_abs, rtol=1e-12, atol=1e-12)          # the two float64 statements of the GCN agree
    assert np.abs(out.detach().cpu().numpy() - out_ref).max() <= 1e-4 * (1.0 + np.abs(out_ref).max())
    for n in names:
        _check(n, got[n], ref[n], terms[n], g["n"] + 2)
        assert np.abs(ref[n]).max() > 1e-3, n


# ---- 8. gcn_norm_edge ------------------------------------------------------------------------------------------------------------
def test_gcn_norm_edge_carries_the_gradient(tfg):
    from tf_geometric_amd.plan import CsrPlan
    g = nm.sweep_graph()
    ei = _dev(np.stack([g["row"], g["col"]]))
    w = _dev(g["w"]).requires_grad_(True)
    index, value = tfg.nn.gcn_norm_edge(ei, g["n"], w)
    E = int(ei.shape[1])
    assert value.requires_grad and tuple(value.shape) == (E + g["n"],) and tuple(index.shape) == (2, E + g["n"])
    perm = CsrPlan.build(ei, g["n"], g["n"]).perm.long()
    ((value[:E].double() * _dev(g["c"])[perm]).sum() + (value[E:].double() * _dev(g["s"])).sum()).backward()
    assert torch.equal(w.grad, _against_float64(g, DEFAULT, g["n"], g["n"]))
