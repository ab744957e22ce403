# coding=utf-8
"""DropEdge on the GPU (include/tfgx_dropedge.h, tfg.nn.drop_edge, tfg.layers.DropEdge): exact agreement with the numpy
mirror of tests/test_drop_edge_abi.py at the compaction tile's edges, the derived plans bit for bit against a rebuilt
(sorted) plan, the hand-over to the layers, seeds, the edge-weight gradient against float64 autograd, the index error and
the example."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_drop_edge_abi import mirror_drop_edge, mirror_plan, _random_edges
from test_gpu_fuzz_backward import _close, _f64

pytestmark = pytest.mark.gpu

TILE = 2048
SIZES = [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
RATES = [0.0, 0.37, 1.0]
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assert_plan_equals_rebuild(tfg, out, plan, what):
    """plan (derived) == CsrPlan.build(out) bit for bit, and == the numpy stable sort; the same for plan._transposed."""
    from tf_geometric_amd.plan import CsrPlan
    for p, ei, tag in ((plan, out, "by dst"), (plan._transposed, torch.stack([out[1], out[0]]), "by src")):
        if p is None:
            continue
        ref = CsrPlan.build(ei.clone(), p.n_dst, p.n_src)
        assert p.num_edges == ref.num_edges == int(out.shape[1]), (what, tag)
        for name in ("row_ptr", "col", "perm"):
            assert torch.equal(getattr(p, name), getattr(ref, name)), "{} {}: {} differs from the rebuilt plan".format(what, tag, name)
        rp, col, perm = mirror_plan(ei.cpu().numpy(), p.n_dst)
        assert np.array_equal(p.row_ptr.cpu().numpy(), rp) and np.array_equal(p.col.cpu().numpy(), col), (what, tag)
        assert np.array_equal(p.perm.cpu().numpy(), perm), (what, tag)


def _with_plan(tfg, ei_np, n_dst, n_src, transposed=True):
    from tf_geometric_amd.plan import CsrPlan
    ei = _dev(ei_np)
    plan = CsrPlan.build(ei, n_dst, n_src)
    if transposed:
        plan.transposed()
    ei._tfgx_plan = plan
    return ei


# ---- 1. against the mirror, exactly -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("rect", [False, True], ids=["square", "rect"])
def test_plain_form_equals_mirror(tfg, E, rate, rect):
    """Few nodes, so duplicate edges and self-loops are everywhere; the rectangular graphs carry a plan (that is how the
    function learns n_dst != n_src), so their derived plans are checked at the tile edges as well."""
    rng = np.random.Generator(np.random.PCG64(1000 + E))
    n_dst, n_src = (29, 61) if rect else (37, 37)
    ei = _random_edges(rng, n_dst, n_src, E)
    if E > 4:
        ei[:, 1], ei[:, 2], ei[1, 3] = ei[:, 0], ei[:, 0], ei[0, 3] % n_src      # duplicates, a self-loop
    w = rng.standard_normal(E).astype(np.float32)
    a2 = rng.standard_normal((3, E)).astype(np.float32)
    ai = rng.integers(0, 9, E).astype(np.int32)
    a64 = rng.standard_normal(E)
    seed = 0xABCDEF0123 + E
    ref_out, ref_id, ref_attrs = mirror_drop_edge(ei, [w, a2, ai, a64, w], rate, seed)
    ei_t = _with_plan(tfg, ei, n_dst, n_src) if rect else _dev(ei)
    got = tfg.nn.drop_edge([ei_t, _dev(w), _dev(a2), _dev(ai), _dev(a64), w], rate=rate, training=True, seed=seed)
    assert len(got) == 6 and got[0].dtype == torch.int32 and tuple(got[0].shape) == ref_out.shape
    assert torch.equal(got[0].cpu(), torch.from_numpy(ref_out))
    for g, r in zip(got[1:5], ref_attrs[:4]):
        assert isinstance(g, torch.Tensor) and g.dtype == torch.from_numpy(r).dtype and tuple(g.shape) == r.shape
        assert torch.equal(g.cpu(), torch.from_numpy(r))
    assert isinstance(got[5], np.ndarray) and np.array_equal(got[5], ref_attrs[4])          # numpy attribute: np.take
    # the kernel's own id output
    from tf_geometric_amd.nn.sampling.drop_edge import drop_edge_index
    out, edge_id, plan = drop_edge_index(ei_t, rate, seed, parent=getattr(ei_t, "_tfgx_plan", None))
    assert torch.equal(edge_id.cpu(), torch.from_numpy(ref_id)) and torch.equal(out.cpu(), torch.from_numpy(ref_out))
    if rect:
        assert plan is not None and got[0]._tfgx_plan is not None
        _assert_plan_equals_rebuild(tfg, got[0], got[0]._tfgx_plan, "E={} rate={}".format(E, rate))
        _assert_plan_equals_rebuild(tfg, out, plan, "E={} rate={} (kernel call)".format(E, rate))
    else:
        assert plan is None and getattr(got[0], "_tfgx_plan", None) is None
    # numpy in -> numpy out
    got_np = tfg.nn.drop_edge([ei, w], rate=rate, training=True, seed=seed)
    assert isinstance(got_np[0], np.ndarray) and got_np[0].dtype == np.int32 and np.array_equal(got_np[0], ref_out)
    assert isinstance(got_np[1], np.ndarray) and np.array_equal(got_np[1], ref_attrs[0])


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("E", SIZES)
def test_undirected_form_equals_mirror(tfg, E, rate):
    rng = np.random.Generator(np.random.PCG64(2000 + E))
    n = 41
    half = _random_edges(rng, n, n, E // 2)
    ei = np.concatenate([half, half[[1, 0]], _random_edges(rng, n, n, E - 2 * (E // 2))], axis=1)     # symmetric (+1 edge when E is odd)
    w, a2 = rng.standard_normal(E).astype(np.float32), rng.standard_normal((2, E)).astype(np.float32)
    seed = 31337 + E
    for name, edges in (("symmetric", ei), ("no upper edge", np.stack([np.maximum(ei[0], ei[1]), np.minimum(ei[0], ei[1])]))):
        ref_out, ref_id, ref_attrs = mirror_drop_edge(edges, [w, a2], rate, seed, force_undirected=True)
        got = tfg.layers.DropEdge(rate, force_undirected=True)([_dev(edges), _dev(w), _dev(a2)], training=True, seed=seed)
        assert torch.equal(got[0].cpu(), torch.from_numpy(ref_out)), name
        assert torch.equal(got[1].cpu(), torch.from_numpy(ref_attrs[0])) and torch.equal(got[2].cpu(), torch.from_numpy(ref_attrs[1])), name
        assert tuple(got[2].shape) == (2, ref_out.shape[1])
        from tf_geometric_amd.nn.sampling.drop_edge import drop_edge_index
        _, edge_id, plan = drop_edge_index(_dev(edges), rate, seed, force_undirected=True)
        assert torch.equal(edge_id.cpu(), torch.from_numpy(ref_id)) and plan is None, name
        if name == "no upper edge":
            assert ref_out.shape == (2, 0) and tuple(got[1].shape) == (0,)


def test_empty_result_keeps_attribute_shapes(tfg):
    ei = _dev(np.stack([np.arange(50), np.arange(50)[::-1]]).astype(np.int32))
    w = torch.ones(50, device=DEV, requires_grad=True)
    out, dw, da = tfg.nn.drop_edge([ei, w, torch.ones(4, 50, device=DEV)], rate=1.0, training=True, seed=1)
    assert tuple(out.shape) == (2, 0) and tuple(dw.shape) == (0,) and tuple(da.shape) == (4, 0)
    dw.sum().backward()
    assert torch.equal(w.grad, torch.zeros_like(w))


# ---- 2. derived plans, bit for bit ----------------------------------------------------------------------------------------------
def _shaped_graph(rng, n_dst, n_src):
    """Rows 0 / 1 / 2 of degree 63 / 64 / 65 (a wave's width and its neighbours), row 3 a hub of 5000 edges (spans tiles),
    rows 4 .. of degree 0-3, the last tenth of the rows without edges; edge order shuffled."""
    deg = np.concatenate([[63, 64, 65, 5000], rng.integers(0, 4, n_dst - 4)])
    deg[n_dst - n_dst // 10:] = 0
    row = np.repeat(np.arange(n_dst), deg)
    col = rng.integers(0, n_src, row.shape[0])
    order = rng.permutation(row.shape[0])
    return np.stack([row[order], col[order]]).astype(np.int32)


@pytest.mark.parametrize("rect", [False, True], ids=["square", "rect"])
@pytest.mark.parametrize("rate", [0.0, 0.5, 0.9, 1.0])
def test_derived_plans_equal_rebuilt_plans(tfg, rate, rect):
    rng = np.random.Generator(np.random.PCG64(77))
    n_dst, n_src = (400, 250) if rect else (400, 400)
    ei = _shaped_graph(rng, n_dst, n_src)
    seed = 2024
    ei_t = _with_plan(tfg, ei, n_dst, n_src)
    out = tfg.nn.drop_edge([ei_t], rate=rate, training=True, seed=seed, derive_plan=True)[0]
    plan = out._tfgx_plan
    assert plan._transposed is not None and plan._transposed._transposed is plan
    assert (plan.n_dst, plan.n_src, plan._transposed.n_dst, plan._transposed.n_src) == (n_dst, n_src, n_src, n_dst)
    _assert_plan_equals_rebuild(tfg, out, plan, "rate={}".format(rate))
    ref_out, _, _ = mirror_drop_edge(ei, [], rate, seed)
    assert torch.equal(out.cpu(), torch.from_numpy(ref_out))
    if rate in (0.5, 0.9):          # the graph must exercise what the issue lists (a property of the seed, checked not assumed)
        before, after = np.bincount(ei[0], minlength=n_dst), np.bincount(ref_out[0], minlength=n_dst)
        assert ((before > 0) & (after == 0)).any(), "no row ended up empty"
        assert (after == 1).any(), "no row with exactly one survivor"
        assert list(before[:4]) == [63, 64, 65, 5000] and after[3] > 0
    # without the parent's transposed plan only the forward plan is derived; the transposed one is built on demand
    ei_f = _with_plan(tfg, ei, n_dst, n_src, transposed=False)
    out_f = tfg.nn.drop_edge([ei_f], rate=rate, training=True, seed=seed, derive_plan=True)[0]
    assert out_f._tfgx_plan._transposed is None
    _assert_plan_equals_rebuild(tfg, out_f, out_f._tfgx_plan, "rate={} forward only".format(rate))
    assert torch.equal(out_f._tfgx_plan.transposed().perm, plan._transposed.perm)
    # the sorted route hands on the same plans
    out_s = tfg.nn.drop_edge([_with_plan(tfg, ei, n_dst, n_src)], rate=rate, training=True, seed=seed, derive_plan=False)[0]
    for a, b in ((out_s._tfgx_plan, plan), (out_s._tfgx_plan._transposed, plan._transposed)):
        assert torch.equal(a.row_ptr, b.row_ptr) and torch.equal(a.col, b.col) and torch.equal(a.perm, b.perm)


def test_parent_plan_from_cache_and_foreign_plan_ignored(tfg):
    from tf_geometric_amd.plan import CsrPlan, CACHE_KEY_PLAN
    rng = np.random.Generator(np.random.PCG64(5))
    ei = _random_edges(rng, 90, 90, 3000)
    cache = {CACHE_KEY_PLAN: CsrPlan.build(_dev(ei), 90, 90)}
    out = tfg.nn.drop_edge([_dev(ei)], rate=0.3, training=True, seed=4, cache=cache)[0]
    _assert_plan_equals_rebuild(tfg, out, out._tfgx_plan, "cache")
    other = {CACHE_KEY_PLAN: CsrPlan.build(_dev(ei[:, :100]), 90, 90)}          # a plan of another list: not used
    out2 = tfg.nn.drop_edge([_dev(ei)], rate=0.3, training=True, seed=4, cache=other)[0]
    assert getattr(out2, "_tfgx_plan", None) is None and torch.equal(out2, out)


# ---- 3. plumbing -------------------------------------------------------------------------------------------------------------------
def test_gcn_on_the_dropped_list_builds_nothing_and_matches_a_sorted_plan(tfg, monkeypatch):
    from tf_geometric_amd.plan import CsrPlan
    rng = np.random.Generator(np.random.PCG64(11))
    n, f = 300, 24
    ei = np.concatenate([_random_edges(rng, n, n, 6000), np.stack([np.full(2500, 7), rng.integers(0, n, 2500)]).astype(np.int32)], 1)
    w = rng.uniform(0.5, 1.5, ei.shape[1]).astype(np.float32)
    x = rng.standard_normal((n, f)).astype(np.float32)
    gout = _dev(rng.standard_normal((n, 16)).astype(np.float32))
    ei_t = _with_plan(tfg, ei, n, n)
    d_ei, d_w = tfg.layers.DropEdge(0.4)([ei_t, _dev(w)], training=True, seed=99)
    assert d_ei._tfgx_plan is not None and d_ei._tfgx_plan._transposed is not None
    layer = tfg.layers.GCN(16, activation=tfg.relu, sym=False).trainable(True)

    def run(edge_index):
        xt = _dev(x).requires_grad_(True)
        out = layer([xt, edge_index, d_w], cache={}, training=True)
        for p in layer.parameters():
            p.grad = None
        out.backward(gout)
        return out.detach().clone(), xt.grad.clone(), [p.grad.clone() for p in layer.parameters()]

    layer._maybe_build([_dev(x)])
    built = []
    real_build = CsrPlan.build
    monkeypatch.setattr(CsrPlan, "build", staticmethod(lambda *a, **k: built.append(1) or real_build(*a, **k)))
    got = run(d_ei)
    assert built == [], "the derived plans were not used: {} sorts".format(len(built))
    ref = run(d_ei.clone())                 # a plain copy carries no plan: the layer sorts (forward and transposed)
    assert len(built) >= 2
    assert torch.equal(got[0], ref[0]), "forward bits differ"
    assert torch.equal(got[1], ref[1]), "d/dx bits differ"
    for a, b in zip(got[2], ref[2]):
        assert torch.equal(a, b), "weight gradient bits differ"


# ---- 4. seeds ------------------------------------------------------------------------------------------------------------------------
def test_seeds(tfg):
    rng = np.random.Generator(np.random.PCG64(21))
    ei = _dev(_random_edges(rng, 500, 500, 3 * TILE + 5))
    a = tfg.nn.drop_edge([ei], rate=0.5, training=True, seed=1234)[0]
    for _ in range(3):
        assert torch.equal(tfg.nn.drop_edge([ei], rate=0.5, training=True, seed=1234)[0], a)
    b = tfg.nn.drop_edge([ei], rate=0.5, training=True, seed=1235)[0]
    assert a.shape != b.shape or not torch.equal(a, b)
    hi = tfg.nn.drop_edge([ei], rate=0.5, training=True, seed=1234 | (1 << 40))[0]          # the upper seed word counts too
    assert a.shape != hi.shape or not torch.equal(a, hi)
    c, d = (tfg.nn.drop_edge([ei], rate=0.5, training=True)[0] for _ in range(2))
    assert c.shape != d.shape or not torch.equal(c, d)
    torch.manual_seed(5)
    e1 = tfg.nn.drop_edge([ei], rate=0.5, training=True)[0]
    torch.manual_seed(5)
    assert torch.equal(tfg.nn.drop_edge([ei], rate=0.5, training=True)[0], e1)                # torch's generator drives seed=None


# ---- 5. gradient ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("und", [False, True], ids=["plain", "undirected"])
def test_edge_weight_gradient_against_float64(tfg, und):
    """d/d edge_weight through drop_edge into a weighted segment sum against float64 autograd of the index restatement, at the
    bar of test_gpu_fuzz_backward for d/dw of a sum: 8 eps sqrt(F) sum|terms|, floor 1e-5."""
    rng = np.random.Generator(np.random.PCG64(31))
    n, F, E = 120, 20, TILE + 700
    ei = _random_edges(rng, n, n, E)
    if und:
        ei = np.concatenate([ei[:, :E // 2], ei[[1, 0], :E // 2]], axis=1)
    w32 = rng.uniform(-1.0, 1.0, E).astype(np.float32)
    x32 = rng.standard_normal((n, F)).astype(np.float32)
    g32 = rng.standard_normal((n, F)).astype(np.float32)
    seed, rate = 4242, 0.4
    ref_out, ref_id, _ = mirror_drop_edge(ei, [], rate, seed, force_undirected=und)
    row, col, idx = (torch.from_numpy(a.astype(np.int64)) for a in (ref_out[0], ref_out[1], ref_id))

    def f(w, x):
        return torch.zeros(n, F, dtype=torch.float64).index_add(0, row, w[idx][:, None] * x[col])

    ref, ref_o = _f64(f, dict(w=w32, x=x32), g32)
    ab, ab_o = _f64(f, dict(w=w32, x=x32), g32, absolute=True)
    w = _dev(w32).requires_grad_(True)
    x = _dev(x32).requires_grad_(True)
    d_ei, d_w = tfg.nn.drop_edge([_dev(ei), w], rate=rate, force_undirected=und, training=True, seed=seed)
    out = tfg.nn.aggregate_neighbors(x, d_ei, d_w, tfg.nn.gcn_mapper, tfg.nn.sum_reducer, tfg.nn.identity_updater)
    out.backward(_dev(g32))
    deg = int(np.bincount(ref_out[0], minlength=n).max(initial=0)) + 2
    _close(out, ref_o.numpy(), ab_o.numpy(), deg, "forward")
    _close(w.grad, ref["w"].numpy(), ab["w"].numpy(), F, "d/dw")
    dropped = np.setdiff1d(np.arange(E), ref_id)
    assert dropped.size and not w.grad.cpu().numpy()[dropped].any()           # dropped edges get exactly zero
    # a [d, E] attribute stays differentiable too
    a2 = _dev(rng.standard_normal((3, E)).astype(np.float32)).requires_grad_(True)
    d_a2 = tfg.nn.drop_edge([_dev(ei), a2], rate=rate, force_undirected=und, training=True, seed=seed)[1]
    coef = _dev(rng.standard_normal(tuple(d_a2.shape)).astype(np.float32))
    (d_a2 * coef).sum().backward()
    want = torch.zeros(3, E, dtype=torch.float32).index_add(1, idx, coef.cpu())
    assert torch.equal(a2.grad.cpu(), want)


# ---- 6. index error ------------------------------------------------------------------------------------------------------------------
def test_out_of_range_endpoint_raises_the_index_error(tfg):
    from tf_geometric_amd._lib import TfgxError
    rng = np.random.Generator(np.random.PCG64(41))
    ei = _random_edges(rng, 50, 50, 3000)
    good = _with_plan(tfg, ei, 50, 50)
    bad = ei.copy()
    bad[1, 2500] = 50                              # one source past the plan's n_src, in the second tile
    bad_t = _dev(bad)
    bad_t._tfgx_plan = good._tfgx_plan
    with pytest.raises(TfgxError, match="code 2.*endpoint outside"):
        tfg.nn.drop_edge([bad_t], rate=0.5, training=True, seed=1)
    neg = ei.copy()
    neg[0, 7] = -1                                 # without a plan the node count is unknown: negative ids are still refused
    for und in (False, True):
        with pytest.raises(TfgxError, match="code 2"):
            tfg.nn.drop_edge([_dev(neg)], rate=0.5, force_undirected=und, training=True, seed=1)
    assert tfg.nn.drop_edge([good], rate=0.5, training=True, seed=1)[0].shape[0] == 2      # the library still works afterwards


def test_bad_attribute_length_is_refused(tfg):
    ei = _dev(np.zeros((2, 10), np.int32))
    with pytest.raises(ValueError, match="last axis"):
        tfg.nn.drop_edge([ei, torch.ones(9, device=DEV)], rate=0.5, training=True)


# ---- 7. example ------------------------------------------------------------------------------------------------------------------------
def test_demo_drop_edge_trains():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "demo_drop_edge.py"), "--nodes", "3000", "--steps", "12"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(line.split("loss")[1].split()[0]) for line in r.stdout.splitlines() if line.startswith("step")]
    # every step sees another random half of the edges, so single steps are noisy: compare the ends of the run
    assert len(losses) == 12 and np.mean(losses[-3:]) < np.mean(losses[:3]), losses
    assert "sorts during training: 0" in r.stdout, r.stdout[-1500:]
