# coding=utf-8
"""ASAP and cluster_pool on the GPU: parity with the reference's own outputs (tests/golden/asap_cases.npz), a seeded fuzz and
the gradients against the float64 mirror (tests/asap_mirror.py, itself held to the golden file by test_asap_reference.py),
the fused attention against the route composed from older operators, the sparse S^T A S against a dense float64 product,
determinism, the plan handed to the next layer, and the public surface.

Bars.  Index outputs and the pooled edge structure are exact.  Sums are held to the aggregation bar of
test_gpu_fuzz_forward.py: assert_parity with 1e-5 * sqrt(max sum of |terms|).  pooled_x = c * act(score) is a product of two
such sums; with |dc| <= t (1 + |c|) and |ds| <= t (1 + |s|) the product is off by at most t [(1 + |c|) |s| + |c| (1 + |s|)]
+ t^2 <= 2 t (1 + |c|) (1 + |s|), which is the bound used (t = that sqrt bar over both sums).  Gradients: the bar of
test_gpu_fuzz_backward.py, per element max(1e-5 (1 + |ref|), 8 * 2^-24 * sqrt(k) * sum|terms|) against float64 autograd on the
mirror, with sum|terms| from the mirror's absolute mode (asap_mirror._Ops: every local Jacobian replaced by its absolute
value, |cotangent| back-propagated) and k the number of terms of the gradient's own reduction."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_parity
import asap_cases as ac
import asap_mirror as am

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "asap_cases.npz")
DEV = "cuda"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_(True) if grad else t


# ---- parity with the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.name)
def test_hip_matches_reference_golden(case, tfg, golden):
    got = case.hip(tfg, case.inputs())
    keys = [k[len(case.name) + 2:] for k in golden if k.startswith(case.name + "::") and not k.endswith("__")]
    assert keys and sorted(keys) == sorted(got)
    for k in keys:
        ref = golden[case.name + "::" + k]
        a = np.asarray(got[k])
        assert a.shape == ref.shape and a.dtype == ref.dtype, "{} {} {} vs {} {}".format(k, a.shape, a.dtype, ref.shape, ref.dtype)
        if a.dtype.kind in "iub":
            assert np.array_equal(a, ref), "{}::{} must be bit-identical to the reference".format(case.name, k)
        else:
            assert_parity(a, ref, tol=ac.TOL, what="{}::{}".format(case.name, k))


# ---- fuzz against the mirror --------------------------------------------------------------------------------------------
def _draw(seed, n=None, graphs=None, F=6, A=4, special=(), weighted=True, kr=None, empty=False):
    """A batch: `graphs` graphs over n nodes (ids shuffled), rows of ordinary degree 0..8 and the `special` degrees on the first
    rows, columns mostly inside the row's graph and some across graphs, self-loops and duplicates."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(rng.integers(40, 401)) if n is None else n
    graphs = int(rng.integers(1, 13)) if graphs is None else graphs
    graphs = min(graphs, n)
    gid = np.concatenate([np.arange(graphs), rng.integers(0, graphs, n - graphs)]).astype(np.int32)
    gid = gid[rng.permutation(n)]
    deg = rng.integers(0, 9, n)
    deg[: len(special)] = special
    rows, cols = [], []
    for i in range(n if not (empty or n == 1) else 0):
        others = np.flatnonzero(np.arange(n) != i)
        same = others[gid[others] == gid[i]]
        pool = same if (same.size and rng.random() < 0.9) else others                            # else: across graphs
        rows.append(np.full(deg[i], i))
        cols.append(rng.choice(pool, deg[i]))                   # never i itself: the row keeps its degree without self-loops
    row = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    if row.size > 8 + sum(special):
        row[-7::2], col[-7::2] = row[-8:-1:2], col[-8:-1:2]      # duplicates (among the last, ordinary rows)
    if row.size:
        loops = rng.integers(0, n, 3).astype(np.int32)           # self-loops: removed by the layer
        row, col = np.concatenate([row, loops]), np.concatenate([col, loops])
    p = rng.permutation(row.size)
    ei = np.stack([row[p], col[p]])
    x = rng.standard_normal((n, F)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, ei.shape[1]).astype(np.float32) if weighted else None
    return dict(seed=seed, n=n, F=F, A=A, x=x, ei=ei, w=w, gid=gid, weights=am.make_weights(rng, F, A),
                kr=kr or dict(ratio=0.5))


DRAWS = [
    dict(seed=1, F=6, A=4, special=(0, 1, 63, 64, 65)),
    dict(seed=2, F=1, A=1, special=(65, 0, 64), weighted=False, kr=dict(k=3)),
    dict(seed=3, F=100, A=16, special=(3000, 0, 1), n=300),
    dict(seed=4, F=260, A=4, special=(63, 130), kr=dict(k=2)),                 # past the fused kernel's width: composed
    dict(seed=5, F=6, A=16, n=1, graphs=1, special=(0,)),                      # N = 1
    dict(seed=6, F=6, A=4, empty=True),                                        # E = 0
    dict(seed=7, F=100, A=1, graphs=1, kr=dict(ratio=1.0)),                    # a graph that keeps all its nodes
    dict(seed=8, F=64, A=4, graphs=12, weighted=False, kr=dict(k=1000)),       # k larger than every graph
    dict(seed=9, F=65, A=16, special=(200,), kr=dict(ratio=0.25)),
    dict(seed=10, F=129, A=4, graphs=3, special=(64, 64, 65)),
    dict(seed=11, F=256, A=16, n=60, kr=dict(k=4)),
    dict(seed=12, F=193, A=1, special=(1, 1, 0, 0), weighted=False),
]


def _spy_topk(monkeypatch):
    """Record the selection asap() makes (it is not part of the return value)."""
    mod = importlib.import_module("tf_geometric_amd.nn.pool.asap")
    seen, real = [], mod.topk_pool

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append(out)
        return out
    monkeypatch.setattr(mod, "topk_pool", spy)
    return seen


def _check_valid_topk(idx, gid, score, kr):
    """Graphs ascending, the right count per graph, and every selected score >= every unselected score of its graph - 1e-5."""
    sel_g = gid[idx]
    assert (np.diff(sel_g) >= 0).all() and np.unique(idx).size == idx.size
    for g in np.unique(gid):
        nodes = np.flatnonzero(gid == g)
        chosen = idx[sel_g == g]
        want = min(kr["k"], nodes.size) if "k" in kr else min(nodes.size, int(np.ceil(np.float32(nodes.size) * np.float32(kr["ratio"]))))
        assert chosen.size == want, (g, chosen.size, want)
        rest = np.setdiff1d(nodes, chosen)
        if chosen.size and rest.size:
            assert score[chosen].min() >= score[rest].max() - 1e-5, (g, score[chosen].min(), score[rest].max())


def _sqrt_bar(*scales):
    return 1e-5 * float(np.sqrt(max([1.0] + [float(s) for s in scales])))


def _check_against_mirror(res, idx, d, act="sigmoid", keep_scale=None):
    m = am.asap_mirror(d["x"], d["ei"], d["w"], d["gid"], d["weights"], activation=act, topk_node_index=idx, keep_scale=keep_scale)
    px, pei, pw, pgi = res
    assert np.array_equal(pc_np(pgi), d["gid"][idx])
    assert pc_np(pei).dtype == np.int32 and np.array_equal(pc_np(pei), m["edge_index"]), "pooled edge structure"
    t = _sqrt_bar(m["c_abs"].max() if m["c_abs"].numel() else 0, m["score_abs"].max() if m["score_abs"].numel() else 0)
    c, s = m["cluster_h"].detach()[torch.from_numpy(idx)].numpy(), m["pooled_score"].detach().numpy()
    bound = 2.0 * t * (1.0 + np.abs(c)) * (1.0 + np.abs(s))
    err = np.abs(pc_np(px).astype(np.float64) - m["x"].detach().numpy())
    assert err.shape == bound.shape and (err <= bound).all(), "pooled_x: max excess {:.3e} (seed {})".format(
        float((err - bound).max()), d["seed"])
    K = idx.size
    assert_parity(pc_np(pw), m["edge_weight"].numpy(), tol=_sqrt_bar(m["P_abs"].max() if K else 0), what="pooled_edge_weight")
    return m


def pc_np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


@pytest.mark.parametrize("cfg", DRAWS, ids=lambda c: "seed{}".format(c["seed"]))
def test_fuzz_against_the_mirror(tfg, cfg, monkeypatch):
    d = _draw(**cfg)
    seen = _spy_topk(monkeypatch)
    names = am.WEIGHT_NAMES
    res = tfg.nn.asap(d["x"], d["ei"], d["w"], d["gid"], *[d["weights"][k] for k in names], None, **d["kr"])
    idx = pc_np(seen[-1]).astype(np.int64)
    free = am.asap_mirror(d["x"], d["ei"], d["w"], d["gid"], d["weights"], **d["kr"])
    _check_valid_topk(idx, d["gid"], free["node_score"].detach().numpy().reshape(-1), d["kr"])
    _check_against_mirror(res, idx, d)


# ---- gradients ----------------------------------------------------------------------------------------------------------
def _host_keep_scale(tfg, seed, rate):
    lib = tfg._lib.load_library()
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))

    def fn(positions):
        return torch.tensor([scale * lib.tfgx_dropout_keep(seed, int(p), rate) for p in positions.tolist()], dtype=torch.float64)
    return fn


@pytest.mark.parametrize("weighted, rate, F, A, special", [(True, 0.0, 24, 8, (0, 1, 65)), (False, 0.0, 100, 4, (130,)),
                                                           (True, 0.3, 24, 8, (0, 64, 70)), (False, 0.3, 7, 1, ())])
def test_gradients_match_float64_autograd(tfg, monkeypatch, weighted, rate, F, A, special):
    d = _draw(seed=40 + F, n=120, graphs=5, F=F, A=A, special=special, weighted=weighted)
    seed = 987654321
    seen = _spy_topk(monkeypatch)
    names = am.WEIGHT_NAMES
    x = _dev(d["x"], grad=True)
    W = {k: _dev(v, grad=True) for k, v in d["weights"].items()}
    res = tfg.nn.asap(x, _dev(d["ei"]), None if d["w"] is None else _dev(d["w"]), _dev(d["gid"]), *[W[k] for k in names], None,
                      ratio=0.5, drop_rate=rate, training=True, seed=seed)
    idx = pc_np(seen[-1]).astype(np.int64)
    rng = np.random.Generator(np.random.PCG64(5))
    G = rng.standard_normal(tuple(res[0].shape)).astype(np.float32)
    (res[0] * _dev(G)).sum().backward()
    keep = _host_keep_scale(tfg, seed, rate) if rate > 0 else None
    _check_against_mirror([t.detach() if isinstance(t, torch.Tensor) else t for t in res], idx, d, keep_scale=keep)

    def mirror_grads(absolute):
        xl = torch.from_numpy(d["x"]).double().requires_grad_(True)
        Wl = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in d["weights"].items()}
        m = am.asap_mirror(xl, d["ei"], d["w"], d["gid"], Wl, topk_node_index=idx, keep_scale=keep, absolute=absolute)
        g = torch.from_numpy(G).double()
        (m["x"] * (g.abs() if absolute else g)).sum().backward()
        return dict(x=xl.grad.numpy(), **{k: Wl[k].grad.numpy() for k in names})
    g64, gabs = mirror_grads(False), mirror_grads(True)
    got = dict(x=x.grad, **{k: W[k].grad for k in names})
    off = d["ei"][:, d["ei"][0] != d["ei"][1]]
    # terms per reduction, as test_gpu_fuzz_backward.py counts them: d/dx sums over the edges that read a row (+ its self
    # edge), a weight gradient over the rows of its operand
    k_of = dict(x=int(np.bincount(off[1], minlength=d["n"]).max(initial=0)) + 1, **{k: d["n"] for k in names})
    for name in ["x"] + names:
        assert got[name] is not None, "no gradient for {}".format(name)
        a, ref, absref = got[name].double().cpu().numpy(), g64[name], gabs[name]
        assert a.shape == ref.shape, name
        assert np.isfinite(a).all(), name
        bound = np.maximum(1e-5 * (1.0 + np.abs(ref)), 8.0 * 2.0 ** -24 * np.sqrt(k_of[name]) * absref)
        err = np.abs(a - ref)
        print("d/d{}: max |ref| {:.3e}, max err {:.3e}, max err / bound {:.3f}".format(
            name, float(np.abs(ref).max()), float(err.max()), float((err / bound).max())))
        assert (err <= bound).all(), "d/d{}: {} of {} elements off, max excess {:.3e}".format(
            name, int((err > bound).sum()), err.size, float((err - bound).max()))
    assert float(np.abs(g64["attention_score_kernel"]).max()) > 0 and float(np.abs(g64["attention_gcn_kernel"]).max()) > 0


# ---- kernel level -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F, rate, special", [(1, 0.0, (0, 1, 63, 64, 65)), (100, 0.0, (3000,)), (256, 0.4, (129, 0)),
                                              (37, 0.4, (64, 65, 1))])
def test_fused_attention_equals_the_composed_route(tfg, F, rate, special):
    from tf_geometric_amd import autograd as AG
    d = _draw(seed=70 + F, n=200, graphs=4, F=F, special=special)
    keep = d["ei"][0] != d["ei"][1]
    ei = _dev(d["ei"][:, keep])
    plan = tfg.CsrPlan.build(ei, d["n"])
    rng = np.random.Generator(np.random.PCG64(F))
    x = _dev(d["x"])
    sq, sh = _dev(rng.standard_normal(d["n"]).astype(np.float32)), _dev(rng.standard_normal(d["n"]).astype(np.float32) * 2)
    b = _dev(np.asarray([0.1], np.float32))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    c, p, p_self, pd, pds = AG.asap_attend_forward(plan, x, sq, sh, b, rate, 77, bad_flag=flag)
    pw, pws = (p, p_self) if pd is None else (pd, pds)
    c2, pw2, pws2 = AG.asap_attend_composed(plan, x, sq, sh, b, rate, 77)
    assert int(flag.item()) == 0
    assert torch.equal(pw == 0, pw2 == 0) and torch.equal(pws == 0, pws2 == 0)            # the same keep mask
    assert_parity(pc_np(pw), pc_np(pw2), what="p")
    assert_parity(pc_np(pws), pc_np(pws2), what="p_self")
    rows = AG.plan_rows(plan)
    terms = torch.zeros(d["n"], F, device=DEV, dtype=torch.float64).index_add(
        0, rows, pw2.double().unsqueeze(1) * x.double().abs()[plan.col.long()]) + pws2.double().unsqueeze(1) * x.double().abs()
    assert_parity(pc_np(c), pc_np(c2), tol=_sqrt_bar(terms.max().item()), what="c")
    sums = torch.zeros(d["n"], device=DEV, dtype=torch.float64).index_add(0, rows, p.double()) + p_self.double()
    assert float((sums - 1.0).abs().max()) < 1e-5                                        # a softmax per row


def test_past_the_width_cap_the_wrapper_takes_the_composed_route(tfg):
    from tf_geometric_amd import autograd as AG
    d = _draw(seed=90, n=50, graphs=2, F=tfg._lib.ASAP_MAX_FEATURES + 4)
    keep = d["ei"][0] != d["ei"][1]
    plan = tfg.CsrPlan.build(_dev(d["ei"][:, keep]), d["n"])
    x, sq, sh = _dev(d["x"]), _dev(d["x"][:, 0].copy()), _dev(d["x"][:, 1].copy())
    b = _dev(np.zeros(1, np.float32))
    got, ref = AG.asap_attend(plan, x, sq, sh, b), AG.asap_attend_composed(plan, x, sq, sh, b)
    for u, v in zip(got, ref):
        assert torch.equal(u, v)
    with pytest.raises(tfg._lib.TfgxError, match="TFGX_ASAP_MAX_FEATURES"):
        AG.asap_attend_forward(plan, x, sq, sh, b)


def _random_assignment(rng, n, K, per_node):
    node = np.repeat(np.arange(n), rng.integers(0, per_node + 1, n)).astype(np.int32)       # 0 .. per_node clusters per node
    cluster = rng.integers(0, K, node.size).astype(np.int32)
    p = rng.permutation(node.size)
    return np.stack([node[p], cluster[p]]), rng.uniform(0.1, 1.0, node.size).astype(np.float32)


@pytest.mark.parametrize("n, K, E, per_node, weighted", [(300, 150, 2000, 3, True), (50, 1, 200, 1, True), (120, 40, 0, 2, True),
                                                         (200, 64, 1500, 4, False), (1, 1, 3, 1, True)])
def test_sparse_sas_equals_dense_float64(tfg, n, K, E, per_node, weighted):
    rng = np.random.Generator(np.random.PCG64(n + K + E))
    ei = rng.integers(0, n, (2, E)).astype(np.int32)
    if E > 10:
        ei[:, 1:10:2] = ei[:, 0:9:2]                                                         # duplicate edges
    w = rng.uniform(0.5, 1.5, E).astype(np.float32) if weighted else None
    assign, aw = _random_assignment(rng, n, K, per_node)
    x = rng.standard_normal((n, 5)).astype(np.float32)
    px, pei, pw = tfg.nn.cluster_pool(x, ei, w, assign, aw if weighted else None, K)
    m = am.cluster_pool_mirror(x, ei, w, assign, aw if weighted else None, K)
    assert isinstance(pei, np.ndarray) and pei.dtype == np.int32 and pw.dtype == np.float32
    assert np.array_equal(pei, m["edge_index"])
    assert_parity(pw, m["edge_weight"].numpy(), tol=_sqrt_bar(m["P_abs"].max()), what="pooled_edge_weight")
    s_abs = np.zeros((n, K))
    np.add.at(s_abs, (assign[0], assign[1]), aw.astype(np.float64) if weighted else 1.0)
    assert_parity(pc_np(px), m["x"].numpy(), tol=_sqrt_bar((s_abs.T @ np.abs(x).astype(np.float64)).max()), what="pooled_x")


def test_unassigned_entries_marked_minus_one_are_skipped(tfg):
    """The kernels' own convention (ASAP uses it instead of compacting): a cluster id outside [0, K) is no entry of S."""
    from tf_geometric_amd.nn.pool.cluster_pool import sparse_sas
    rng = np.random.Generator(np.random.PCG64(3))
    n, K, E = 80, 20, 600
    ei = rng.integers(0, n, (2, E)).astype(np.int32)
    assign, aw = _random_assignment(rng, n, K, 3)
    drop = rng.random(assign.shape[1]) < 0.3
    plan = tfg.CsrPlan.build(_dev(assign), n, K)
    s_col = plan.col.clone()
    marked = _dev(drop)[plan.perm.long()]
    s_col[marked] = -1
    row, col, val, row_ptr = sparse_sas(plan.row_ptr, s_col, plan.edge_attr_to_csr(_dev(aw)), n, K, _dev(ei[0].copy()),
                                        _dev(ei[1].copy()), None)
    m = am.cluster_pool_mirror(None, ei, None, assign[:, ~drop], aw[~drop], K, num_nodes=n)
    assert np.array_equal(np.stack([pc_np(row), pc_np(col)]), m["edge_index"])
    assert_parity(pc_np(val), m["edge_weight"].numpy(), tol=_sqrt_bar(m["P_abs"].max()), what="values")
    assert np.array_equal(pc_np(row_ptr), np.concatenate([[0], np.cumsum(np.bincount(m["edge_index"][0], minlength=K))]))


# ---- determinism --------------------------------------------------------------------------------------------------------
def test_determinism(tfg):
    d = _draw(seed=21, n=300, graphs=6, F=100, A=16, special=(3000, 64, 65))

    def run():
        x = _dev(d["x"], grad=True)
        W = {k: _dev(v, grad=True) for k, v in d["weights"].items()}
        out = tfg.nn.asap(x, _dev(d["ei"]), _dev(d["w"]), _dev(d["gid"]), *[W[k] for k in am.WEIGHT_NAMES], None, ratio=0.5,
                          drop_rate=0.2, training=True, seed=11)
        (out[0] * torch.arange(out[0].numel(), device=DEV, dtype=torch.float32).reshape(out[0].shape).sin()).sum().backward()
        return [t.detach().clone() for t in out] + [x.grad.clone()] + [W[k].grad.clone() for k in am.WEIGHT_NAMES]

    a, b = run(), run()
    assert len(a) == 4 + 1 + 11
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_cluster_pool_determinism(tfg):
    rng = np.random.Generator(np.random.PCG64(17))
    n, K, E = 300, 90, 3000
    ei = rng.integers(0, n, (2, E)).astype(np.int32)
    w = rng.uniform(0.5, 1.5, E).astype(np.float32)
    assign, aw = _random_assignment(rng, n, K, 4)
    x_np = rng.standard_normal((n, 33)).astype(np.float32)

    def run():
        x = _dev(x_np, grad=True)
        px, pei, pw = tfg.nn.cluster_pool(x, _dev(ei), _dev(w), _dev(assign), _dev(aw), K)
        (px * torch.arange(px.numel(), device=DEV, dtype=torch.float32).reshape(px.shape).cos()).sum().backward()
        return [px.detach().clone(), pei.clone(), pw.clone(), x.grad.clone()]

    for u, v in zip(run(), run()):
        assert torch.equal(u, v)


# ---- the plan handed on -------------------------------------------------------------------------------------------------
def test_pooled_edge_index_carries_the_plan_a_rebuild_gives(tfg):
    d = _draw(seed=31, n=250, graphs=5, F=16, A=4, special=(65, 0))
    args = [_dev(d["x"]), _dev(d["ei"]), _dev(d["w"]), _dev(d["gid"])] + [_dev(d["weights"][k]) for k in am.WEIGHT_NAMES] + [None]
    px, pei, pw, pgi = tfg.nn.asap(*args, ratio=0.5)
    assert all(isinstance(t, torch.Tensor) for t in (px, pei, pw, pgi))                   # tensor in -> tensor out
    K = int(px.shape[0])
    plan = pei._tfgx_plan
    assert tfg.CsrPlan.from_cache(pei, K) is plan and tfg.SparseMatrix(pei, pw, [K, K]).plan is plan
    rebuilt = tfg.CsrPlan.build(pei.clone(), K)
    assert (plan.n_dst, plan.n_src, plan.num_edges) == (rebuilt.n_dst, rebuilt.n_src, rebuilt.num_edges)
    for a in ("row_ptr", "col", "perm"):
        assert torch.equal(getattr(plan, a), getattr(rebuilt, a)), a
    gcn = tfg.layers.GCN(8, seed=1)
    with_plan = gcn([px, pei, pw])
    without = gcn([px, pei.clone(), pw])
    assert torch.equal(with_plan, without)
    # a second level straight on the pooled graph: the attached plan has self-loops to remove, so it is rebuilt, not misused
    args2 = [px, pei, pw, pgi] + [_dev(am.make_weights(np.random.default_rng(2), 16, 4)[k]) for k in am.WEIGHT_NAMES] + [None]
    again = tfg.nn.asap(*args2, ratio=0.5)
    fresh = tfg.nn.asap(px, pei.clone(), pw, pgi, *args2[4:], ratio=0.5)
    for u, v in zip(again, fresh):
        assert torch.equal(u, v)


def test_cache_gives_the_same_bits_and_numpy_gives_numpy(tfg):
    d = _draw(seed=33, n=90, graphs=3, F=8, A=4)
    ws = [d["weights"][k] for k in am.WEIGHT_NAMES] + [None]
    cache = {}
    a = tfg.nn.asap(d["x"], d["ei"], d["w"], d["gid"], *ws, k=5, cache=cache)
    b = tfg.nn.asap(d["x"], d["ei"], d["w"], d["gid"], *ws, k=5, cache=cache)
    c = tfg.nn.asap(d["x"], d["ei"], d["w"], d["gid"], *ws, k=5)
    assert "tfgx_asap" in cache
    assert all(isinstance(t, np.ndarray) for t in a[1:]) and a[1].dtype == np.int32 and a[2].dtype == np.float32
    for u, v, z in zip(a, b, c):
        assert np.array_equal(pc_np(u), pc_np(v)) and np.array_equal(pc_np(u), pc_np(z))


# ---- the public surface -------------------------------------------------------------------------------------------------
def test_layer_weights_names_shapes_and_losses(tfg):
    d = _draw(seed=35, n=60, graphs=2, F=12, A=5)
    layer = tfg.layers.ASAP(ratio=0.5, attention_units=5, kernel_regularizer=lambda w: (w * w).sum(),
                            bias_regularizer=lambda w: w.abs().sum())
    inputs = [_dev(d["x"]), _dev(d["ei"]), _dev(d["w"]), _dev(d["gid"])]
    layer._maybe_build(inputs)
    shapes = {k: tuple(v.shape) for k, v in layer.weights.items()}
    assert shapes == dict(attention_gcn_kernel=(12, 5), attention_gcn_bias=(5,), attention_query_kernel=(5, 5),
                          attention_query_bias=(5,), attention_score_kernel=(10, 1), attention_score_bias=(1,),
                          le_conv_self_kernel=(12, 1), le_conv_self_bias=(1,), le_conv_aggr_self_kernel=(12, 1),
                          le_conv_aggr_self_bias=(1,), le_conv_aggr_neighbor_kernel=(12, 1))
    assert list(shapes) == am.WEIGHT_NAMES and float(layer.attention_gcn_bias.abs().max()) == 0.0
    assert len(layer.losses) == 11
    layer.set_weights(**d["weights"])
    got = layer(inputs)
    ref = tfg.nn.asap(*inputs, *[_dev(d["weights"][k]) for k in am.WEIGHT_NAMES], None, ratio=0.5)
    for u, v in zip(got, ref):
        assert torch.equal(u, v)
    nobias = tfg.layers.ASAP(k=2, le_conv_use_bias=False)
    nobias._maybe_build(inputs)
    assert len(nobias.weights) == 9 and nobias.le_conv_self_bias is None and len(nobias(inputs)) == 4


def test_cluster_pool_refusals_and_x_gradient(tfg):
    d = _draw(seed=36, n=40, graphs=2, F=4)
    rng = np.random.Generator(np.random.PCG64(1))
    assign, aw = _random_assignment(rng, d["n"], 6, 2)
    with pytest.raises(Exception, match="Please provide num_nodes if x is None"):
        tfg.nn.cluster_pool(None, d["ei"], None, assign, None, 6)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        tfg.nn.cluster_pool(d["x"], _dev(d["ei"]), None, _dev(assign), _dev(aw, grad=True), 6)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        tfg.nn.cluster_pool(d["x"], _dev(d["ei"]), _dev(d["w"], grad=True), _dev(assign), None, 6)
    x = _dev(d["x"], grad=True)
    px, pei, pw = tfg.nn.cluster_pool(x, _dev(d["ei"]), _dev(d["w"]), _dev(assign), _dev(aw), 6)
    assert isinstance(pei, torch.Tensor) and pw.requires_grad is False
    px.sum().backward()
    ref = np.zeros(d["n"])
    np.add.at(ref, assign[0], aw.astype(np.float64))
    assert_parity(pc_np(x.grad), np.repeat(ref[:, None], 4, axis=1), what="d pooled_x / dx")
    out = tfg.nn.cluster_pool(None, d["ei"], None, assign, None, 6, num_nodes=d["n"])
    assert out[0] is None and out[1].shape[0] == 2


def test_refused_inside_graph_capture(tfg):
    d = _draw(seed=37, n=30, graphs=2)
    args = [_dev(d["x"]), _dev(d["ei"]), None, _dev(d["gid"])] + [_dev(d["weights"][k]) for k in am.WEIGHT_NAMES] + [None]
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with pytest.raises(RuntimeError, match="capture"):
            with torch.cuda.graph(graph, stream=side):
                tfg.nn.asap(*args, k=2)
    torch.cuda.synchronize()


def test_dense_converters(tfg):
    adj = np.asarray([[0.0, 2.0, 0.0], [0.0, 0.0, -1.0], [3.0, 0.0, 4.0]], np.float32)
    ei, w = tfg.utils.convert_dense_adj_to_edge(adj)
    assert isinstance(ei, np.ndarray) and ei.dtype == np.int32
    assert np.array_equal(ei, [[0, 1, 2, 2], [1, 2, 0, 2]]) and np.array_equal(w, np.asarray([2, -1, 3, 4], np.float32))
    tei, tw = tfg.utils.convert_dense_adj_to_edge(torch.from_numpy(adj).to(DEV))
    assert isinstance(tei, torch.Tensor) and np.array_equal(pc_np(tei), ei) and np.array_equal(pc_np(tw), w)
    s = np.arange(6, dtype=np.float32).reshape(3, 2)
    aei, aw = tfg.utils.convert_dense_assign_to_edge(s)
    assert np.array_equal(aei, [[0, 0, 1, 1, 2, 2], [0, 1, 0, 1, 0, 1]]) and np.array_equal(aw, s.reshape(-1))
    aei, aw = tfg.utils.convert_dense_assign_to_edge(s, node_graph_index=np.asarray([0, 2, 1], np.int32))
    assert np.array_equal(aei[1], [0, 1, 4, 5, 2, 3]) and aei.dtype == np.int32
    # the dense route and the sparse route of cluster_pool agree
    rng = np.random.Generator(np.random.PCG64(4))
    S = (rng.random((30, 5)) * (rng.random((30, 5)) < 0.4)).astype(np.float32)
    ei = rng.integers(0, 30, (2, 100)).astype(np.int32)
    aei, aw = tfg.utils.convert_dense_assign_to_edge(S)
    _, pei, pw = tfg.nn.cluster_pool(None, ei, None, aei, aw, 5, num_nodes=30)
    A = np.zeros((30, 30))
    np.add.at(A, (ei[0], ei[1]), 1.0)
    dei, dw = tfg.utils.convert_dense_adj_to_edge((S.astype(np.float64).T @ A @ S.astype(np.float64)).astype(np.float32))
    assert np.array_equal(pei, dei)
    assert_parity(pw, dw, tol=_sqrt_bar(np.abs(dw).max()), what="S^T A S")


# ---- the hierarchical model ---------------------------------------------------------------------------------------------
def test_asap_model_trains(tfg):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import demo_asap as demo
    data = demo.make_dataset(num_graphs=256, seed=0)
    model = demo.ASAPModel(data.num_features, data.num_classes, seed=0)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    batch = demo.make_batch(data, list(range(128)))
    losses = [demo.train_step(model, opt, batch) for _ in range(15)]
    assert all(np.isfinite(losses))
    assert np.mean(losses[-3:]) < np.mean(losses[:3]) - 0.03, losses
