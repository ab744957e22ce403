# coding=utf-8
"""Link prediction on the GPU (include/tfgx_linkpred.h): tfg.nn.edge_dot forward against float64 numpy and backward
against float64 torch autograd of the gather form, with tolerances DERIVED from the classical dot-product bound (never
tuned); both negative samplers against the numpy mirror of tests/test_linkpred_abi.py bit for bit; the without-replacement
rounds, the dense-graph fallback, the error paths and the example's training loop."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_linkpred_abi import (GRAPH8, N8, mirror_pairs, mirror_from, mirror_without_replacement, upper_edge_set,
                               directed_edge_set)

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24        # unit roundoff of float32
N_A, N_B = 37, 23
EDGE_COUNTS = (1, 15, 16, 17, 63, 64, 65, 1000)


def _table(rng, n, F, ld):
    """A float32 [n, F] view with row stride ld on the GPU, and its float64 numpy copy."""
    base = torch.zeros((n, ld), dtype=torch.float32, device="cuda")
    vals = rng.standard_normal((n, F)).astype(np.float32)
    base[:, :F] = torch.from_numpy(vals).cuda()
    return base[:, :F], vals.astype(np.float64)


def _edges(rng, E, n_a, n_b):
    ei = np.stack([rng.integers(0, n_a, E), rng.integers(0, n_b, E)]).astype(np.int32)
    if E >= 16:
        ei[:, 3] = ei[:, 9]                        # a duplicate edge
        ei[:, 5] = min(n_a, n_b) - 1               # a self-pair (of the shared table)
    return ei


def _check_forward(got, a64, b64, ei, F, what):
    prod = a64[ei[0]] * b64[ei[1]]
    ref = prod.sum(-1)
    bound = (F + 3) * U24 * np.abs(prod).sum(-1)   # |fl(sum) - sum| <= gamma_F sum |a_f b_f| for ANY summation order
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all(), "{}: worst err / bound = {:.3f}".format(what, float((err / np.maximum(bound, 1e-300)).max()))


@pytest.mark.parametrize("layout", ["aligned", "padded"])
@pytest.mark.parametrize("F", [1, 3, 4, 16, 47, 64, 65, 100, 256, 300])
def test_edge_dot_forward_against_float64(tfg, F, layout):
    """aligned: row stride = F rounded up to 4 (16-byte loads when F % 4 == 0); padded: stride F + 1 (the 4-byte path)."""
    rng = np.random.Generator(np.random.PCG64(1000 + F))
    ld = (F + 3) // 4 * 4 if layout == "aligned" else F + 1
    z, z64 = _table(rng, N_A, F, ld)
    zo, zo64 = _table(rng, N_B, F, ld)
    assert z.stride(0) == ld
    for E in EDGE_COUNTS:
        ei = _edges(rng, E, N_A, N_B)
        ei_t = torch.from_numpy(ei).cuda()
        got = tfg.nn.edge_dot(z, ei_t, zo)
        assert got.shape == (E,) and got.dtype == torch.float32
        _check_forward(got.cpu().numpy(), z64, zo64, ei, F, "separate F={} E={}".format(F, E))
        assert torch.equal(got, tfg.nn.edge_dot(z, ei_t, zo)), "two runs differ"
        ei_s = _edges(rng, E, N_B, N_B)             # one shared table: a == b
        got_s = tfg.nn.edge_dot(zo, ei_s)           # numpy edge_index in, tensor out
        _check_forward(got_s.cpu().numpy(), zo64, zo64, ei_s, F, "shared F={} E={}".format(F, E))
        assert torch.equal(got_s, tfg.nn.edge_dot(zo, torch.from_numpy(ei_s).cuda()))
    assert tfg.nn.edge_dot(z, np.zeros((2, 0), np.int32), zo).shape == (0,)


def test_edge_dot_out_of_range_endpoint(tfg):
    from tf_geometric_amd import autograd as AG
    rng = np.random.Generator(np.random.PCG64(7))
    F = 20
    z, z64 = _table(rng, N_A, F, F)
    zo, zo64 = _table(rng, N_B, F, F)
    ei = _edges(rng, 100, N_A, N_B)
    bad = {11: (N_A, 0), 40: (0, N_B), 77: (-1, 3), 99: (2, -5)}
    for e, (r, c) in bad.items():
        ei[:, e] = (r, c)
    ei_t = torch.from_numpy(ei).cuda()
    with pytest.raises(tfg._lib.TfgxError, match="code 2"):
        tfg.nn.edge_dot(z, ei_t, zo)
    with pytest.raises(tfg._lib.TfgxError, match="code 2"):
        tfg.nn.edge_dot(z, ei_t, zo)                # not memoised as checked
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = AG.edge_dot_forward(z, zo, ei_t[0].contiguous(), ei_t[1].contiguous(), bad_flag=flag).cpu().numpy()
    assert int(flag.item()) == 1
    good = np.array([e for e in range(100) if e not in bad])
    assert (out[list(bad)] == 0.0).all()
    _check_forward(out[good], z64, zo64, ei[:, good], F, "good edges next to bad ones")
    ok = torch.from_numpy(ei[:, good]).cuda()
    tfg.nn.edge_dot(z, ok, zo)
    assert ok._tfgx_edge_dot_range == (ok._version, N_A, N_B)      # read once per edge_index tensor


def _backward_case(rng, shared, F):
    n_a, n_b = (40, 40) if shared else (40, 29)
    E = 700
    ei = np.stack([rng.integers(0, n_a, E), rng.integers(0, n_b, E)]).astype(np.int32)
    ei[0, ei[0] == 7] = 8                           # row 7: degree 0
    ei[0, :300][ei[0, :300] != 5] = 5
    ei[0, 300:][ei[0, 300:] == 5] = 6               # row 5: degree exactly 300
    ei = ei[:, rng.permutation(E)]
    assert (ei[0] == 5).sum() == 300 and (ei[0] == 7).sum() == 0
    z = rng.standard_normal((n_a, F)).astype(np.float32)
    zo = z if shared else rng.standard_normal((n_b, F)).astype(np.float32)
    g = rng.standard_normal(E).astype(np.float32)
    return ei, z, zo, g


def _reference_grads(ei, z, zo, g, shared):
    """float64 torch autograd of (z[row] * z_other[col]).sum(-1), and the derived per-entry bounds:
    dz[i, f] = sum_{e: row = i} g_e zo[col_e, f] is a dot product of deg_i terms (formed as g_e * zo in float32, then
    summed in some order): |err| <= (deg_i + 3) 2^-24 sum_e |g_e| |zo[col_e, f]|; likewise for d z_other over the
    edges that share a column.  Shared table: the result is the float32 sum of the two, so the two bounds add, plus one
    rounding of that last addition, at most 2^-24 (1 + 2^-20) (sum_e |..| + sum_e |..|)  (the partial sums are bounded by
    their absolute sums up to their own error, which the factor 1 + 2^-20 covers for deg <= 2^16)."""
    row, col = torch.from_numpy(ei[0]).long(), torch.from_numpy(ei[1]).long()
    z64 = torch.from_numpy(z).double().requires_grad_(True)
    zo64 = z64 if shared else torch.from_numpy(zo).double().requires_grad_(True)
    (z64[row] * zo64[col]).sum(-1).backward(torch.from_numpy(g).double())
    ag = np.abs(g.astype(np.float64))[:, None]
    abs_a = np.zeros(z.shape, np.float64)
    np.add.at(abs_a, ei[0], ag * np.abs(zo.astype(np.float64))[ei[1]])
    abs_b = np.zeros(zo.shape, np.float64)
    np.add.at(abs_b, ei[1], ag * np.abs(z.astype(np.float64))[ei[0]])
    deg_a = np.bincount(ei[0], minlength=z.shape[0])[:, None]
    deg_b = np.bincount(ei[1], minlength=zo.shape[0])[:, None]
    bound_a, bound_b = (deg_a + 3) * U24 * abs_a, (deg_b + 3) * U24 * abs_b
    if shared:
        return (z64.grad.numpy(),), (bound_a + bound_b + U24 * (1 + 2.0 ** -20) * (abs_a + abs_b),)
    return (z64.grad.numpy(), zo64.grad.numpy()), (bound_a, bound_b)


@pytest.mark.parametrize("F", [16, 47])
@pytest.mark.parametrize("shared", [True, False])
def test_edge_dot_backward_against_float64_autograd(tfg, shared, F):
    from tf_geometric_amd.plan import CsrPlan, CACHE_KEY_PLAN
    rng = np.random.Generator(np.random.PCG64(50 + F + int(shared)))
    ei, z, zo, g = _backward_case(rng, shared, F)
    refs, bounds = _reference_grads(ei, z, zo, g, shared)
    g_t = torch.from_numpy(g).cuda()

    def run(source):
        ei_t = torch.from_numpy(ei).cuda()
        cache = None
        if source == "cache":
            cache = {CACHE_KEY_PLAN: CsrPlan.build(ei_t, z.shape[0], zo.shape[0])}
        elif source == "attached":
            ei_t._tfgx_plan = CsrPlan.build(ei_t, z.shape[0], zo.shape[0])
        zt = torch.from_numpy(z).cuda().requires_grad_(True)
        zot = None if shared else torch.from_numpy(zo).cuda().requires_grad_(True)
        out = tfg.nn.edge_dot(zt, ei_t, zot, cache=cache)
        _check_forward(out.detach().cpu().numpy(), z.astype(np.float64), zo.astype(np.float64), ei, F, "forward with grad")
        out.backward(g_t)
        if source == "fresh":
            assert isinstance(ei_t._tfgx_plan, CsrPlan)            # one build, memoised on the tensor
            built = ei_t._tfgx_plan
            tfg.nn.edge_dot(zt, ei_t, zot).backward(g_t)
            assert ei_t._tfgx_plan is built
            zt.grad = None if zt.grad is None else zt.grad / 2     # two identical passes were accumulated (exact halving)
            if zot is not None:
                zot.grad = zot.grad / 2
        return [t.grad.clone() for t in ((zt,) if shared else (zt, zot))]

    first = run("cache")
    for got, ref, bound in zip(first, refs, bounds):
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        assert (err <= bound).all(), "worst err / bound = {:.3f}".format(float((err / np.maximum(bound, 1e-300)).max()))
    assert float(first[0][7].abs().max()) == 0.0 or shared         # the row of degree 0 (its own gradient part)
    for source in ("cache", "attached", "fresh"):
        again = run(source)
        for a, b in zip(first, again):
            assert torch.equal(a, b), "gradients differ between runs / plan sources ({})".format(source)


def test_edge_dot_refuses_a_plan_of_another_list(tfg):
    from tf_geometric_amd.plan import CsrPlan, CACHE_KEY_PLAN
    z = torch.randn(10, 8, device="cuda", requires_grad=True)
    other = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32, device="cuda")
    ei = torch.tensor([[0, 1], [3, 4]], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="plan"):
        tfg.nn.edge_dot(z, ei, cache={CACHE_KEY_PLAN: CsrPlan.build(other, 10, 10)})


# ---- samplers ------------------------------------------------------------------------------------------------------------
def _random_graph(seed, n, e):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.stack([rng.integers(0, n, e), rng.integers(0, n, e)]).astype(np.int32)


@pytest.fixture(scope="module")
def graph1000():
    ei = _random_graph(3, 1000, 5000)
    return ei, upper_edge_set(ei), directed_edge_set(ei)


def test_negative_sampling_equals_the_mirror_small_graph(tfg):
    edges = upper_edge_set(GRAPH8)
    got = tfg.utils.negative_sampling(2000, N8, GRAPH8, seed=2024)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32
    assert got.tolist() == mirror_pairs(2000, N8, edges, 2024).tolist()
    t = torch.from_numpy(GRAPH8).cuda()
    got_t = tfg.utils.negative_sampling(2000, N8, t, seed=2024)
    assert isinstance(got_t, torch.Tensor) and got_t.cpu().numpy().tolist() == got.tolist()
    assert t._tfgx_adjacency[1][(N8, True)][2] == 10               # the adjacency is memoised on the tensor
    both = np.concatenate([GRAPH8, GRAPH8[::-1]], axis=1)
    start = (np.arange(3000) % N8).astype(np.int32)
    pairs = tfg.utils.negative_sampling_with_start_node(start, N8, both, seed=99)
    assert pairs.shape == (2, 3000) and pairs[0].tolist() == start.tolist()
    assert pairs[1].tolist() == mirror_from(start, N8, directed_edge_set(both), 99).tolist()


def test_negative_sampling_equals_the_mirror_n1000(tfg, graph1000):
    ei, upper, directed = graph1000
    got = tfg.utils.negative_sampling(4096, 1000, ei, seed=11)
    assert got.tolist() == mirror_pairs(4096, 1000, upper, 11).tolist()
    assert (got[0] < got[1]).all()
    batches = tfg.utils.negative_sampling(300, 1000, ei, batch_size=3, seed=11)
    assert len(batches) == 3 and batches[0].tolist() == got[:, :300].tolist()
    assert batches[2].tolist() == mirror_pairs(300, 1000, upper, 11, slot_base=2 << 40).tolist()      # disjoint windows
    rng = np.random.Generator(np.random.PCG64(5))
    start = rng.integers(0, 1000, 4096).astype(np.int32)
    pairs = tfg.utils.negative_sampling_with_start_node(torch.from_numpy(start).cuda(), 1000, ei, seed=12)
    assert isinstance(pairs, torch.Tensor)
    assert pairs[1].cpu().numpy().tolist() == mirror_from(start, 1000, directed, 12).tolist()


def test_negative_sampling_without_filter_and_with_a_slot_base(tfg, graph1000):
    from tf_geometric_amd.utils import link
    got = tfg.utils.negative_sampling(1500, 1000, seed=21)
    assert isinstance(got, np.ndarray) and got.tolist() == mirror_pairs(1500, 1000, None, 21).tolist()
    ends = tfg.utils.negative_sampling_with_start_node(np.zeros(1500, np.int32), 1000, seed=21)
    assert ends[1].tolist() == got[1].tolist()
    ei, upper, _ = graph1000
    adj = tfg.utils.sorted_adjacency(ei, 1000, undirected=True)
    n_failed = torch.zeros(1, dtype=torch.int32, device="cuda")
    for base in (12345, (1 << 33) + 7):
        out = link._launch_pairs(700, 1000, adj, True, 31, base, n_failed, n_failed.device)
        assert out.cpu().numpy().tolist() == mirror_pairs(700, 1000, upper, 31, slot_base=base).tolist()
    assert int(n_failed.item()) == 0


def test_sorted_adjacency_layout(tfg, graph1000):
    ei, upper, directed = graph1000
    for undirected, edges in ((True, upper), (False, {e for e in directed if e[0] != e[1]})):
        ptr, col, U = tfg.utils.sorted_adjacency(ei, 1000, undirected=undirected)
        ptr, col = ptr.cpu().numpy(), col.cpu().numpy()[:U]
        assert U == len(edges) and ptr[0] == 0 and ptr[-1] == U and ptr.shape == (1001,)
        rows = np.repeat(np.arange(1000), np.diff(ptr))
        assert set(zip(rows.tolist(), col.tolist())) == edges
        key = rows.astype(np.int64) * 1000 + col
        assert (np.diff(key) > 0).all()                            # strictly ascending inside every row
    with pytest.raises(tfg._lib.TfgxError, match="code 2"):
        tfg.utils.sorted_adjacency(np.array([[0, 5], [1, 1000]], np.int32), 1000)


def test_negative_sampling_without_replacement_over_two_rounds(tfg):
    from tf_geometric_amd.utils import link
    ei = _random_graph(8, 40, 120)
    edges = upper_edge_set(ei)
    non_edges = 40 * 39 // 2 - len(edges)
    want = int(0.9 * non_edges)
    rounds = link.STATS["rounds"]
    got = tfg.utils.negative_sampling(want, 40, ei, replace=False, seed=77)
    assert link.STATS["rounds"] - rounds >= 2
    assert got.shape == (2, want) and len(set(map(tuple, got.T.tolist()))) == want
    assert got.tolist() == mirror_without_replacement(want, 40, edges, 77).tolist()
    every = tfg.utils.negative_sampling(18, N8, GRAPH8, replace=False, seed=4)
    assert every.tolist() == mirror_without_replacement(18, N8, upper_edge_set(GRAPH8), 4).tolist()
    launches = link.STATS["launches"]
    with pytest.raises(ValueError):
        tfg.utils.negative_sampling(19, N8, GRAPH8, replace=False, seed=4)
    assert link.STATS["launches"] == launches                      # refused before any launch
    with pytest.raises(NotImplementedError):
        tfg.utils.negative_sampling(5, N8, GRAPH8, mode="directed")


def test_negative_sampling_dense_graph_fallback(tfg):
    from tf_geometric_amd.utils import link
    full = np.array([(a, b) for a in range(6) for b in range(a + 1, 6) if (a, b) != (2, 4)], dtype=np.int32).T
    before = link.STATS["dense_fallback"]
    got = tfg.utils.negative_sampling(5, 6, full, seed=1)
    assert link.STATS["dense_fallback"] == before + 1
    assert got.shape == (2, 5) and got.dtype == np.int32 and (got == np.array([[2], [4]])).all()
    assert tfg.utils.negative_sampling(1, 6, full, replace=False, seed=1).tolist() == [[2], [4]]
    with pytest.raises(ValueError):
        tfg.utils.negative_sampling(2, 6, full, replace=False, seed=1)
    complete = np.array([(a, b) for a in range(6) for b in range(a + 1, 6)], dtype=np.int32).T
    with pytest.raises(ValueError):
        tfg.utils.negative_sampling(1, 6, complete, seed=1)


def test_start_node_errors(tfg):
    both = np.concatenate([GRAPH8, GRAPH8[::-1]], axis=1)
    with pytest.raises(tfg._lib.TfgxError, match="code 2"):
        tfg.utils.negative_sampling_with_start_node(np.array([0, 8, 1], np.int32), N8, both, seed=1)
    with pytest.raises(tfg._lib.TfgxError, match="code 2"):
        tfg.utils.negative_sampling_with_start_node(np.array([-1], np.int32), N8, seed=1)
    star = np.array([[0] * 7, list(range(1, 8))], np.int32)        # node 0 is linked to everyone: it has no non-neighbour
    with pytest.raises(RuntimeError, match="non-neighbour"):
        tfg.utils.negative_sampling_with_start_node(np.array([0], np.int32), N8, star, seed=1)


def test_demo_gae_loop_trains(tfg, capsys):
    spec = importlib.util.spec_from_file_location("demo_gae", os.path.join(ROOT, "examples", "demo_gae.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    losses, auc = demo.main(nodes=200, steps=30, seed=0, verbose=False)
    with capsys.disabled():
        print("demo_gae n=200: loss {:.4f} -> {:.4f}, test AUC {:.4f}".format(losses[0], losses[-1], auc))
    assert len(losses) == 30 and all(np.isfinite(losses))
    assert losses[-1] < losses[0]
