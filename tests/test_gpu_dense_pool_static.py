# coding=utf-8
"""DiffPool and MinCutPool on fixed-shape batches (include/tfgx_dense_pool_static.h, nn/pool/dense_pool_static.py) on the GPU:
the layout against the numpy mirror, exactly; the live part against the eager route, bit for bit; a two-level model against
float64 autograd with inert padding; the MinCut losses; no host read and no sort; capture and replay; composition with the
other static pools; refusals; the two examples."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from densepool_static_mirror import mirror_dense_pool_static, mirror_pooled_weight
from test_collate_abi import random_dataset
from test_gpu_collate import _eq, _plan_eq
from test_gpu_nbrblock import _close

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = 5
sys.path.insert(0, os.path.join(ROOT, "examples"))

# a dozen graphs of 0-40 (nodes, edges): an empty one, one without edges, some with fewer nodes than K = 3 / 20 / 64
SIZES = [(0, 0), (1, 1), (2, 3), (3, 5), (7, 12), (33, 70), (40, 90), (6, 0), (12, 30), (25, 60), (17, 40), (5, 8)]
EMPTY, NO_EDGES = 0, 7
BATCHES = {"dead slots last": [5, EMPTY, NO_EDGES, 2, 9, -1, -1],
           "dead slots interleaved": [-1, 5, -1, EMPTY, NO_EDGES, 6, -1, 1, 4, -1],
           "all slots dead": [-1, -1, -1]}
_WORLD = {}


def _world():
    """(GraphStore, its packed arrays): built once and left unchanged."""
    if "w" not in _WORLD:
        import tf_geometric_amd as tfg
        d = random_dataset(np.random.Generator(np.random.PCG64(177)), SIZES, F, y=False)
        d["y"] = (np.arange(len(SIZES), dtype=np.int64) % 3).reshape(-1, 1)
        _WORLD["w"] = (tfg.data.GraphStore.from_arrays(**d), d)
    return _WORLD["w"]


def _ids(ids):
    return torch.tensor(ids, dtype=torch.int32, device=DEV)


def _rebuilt(ei, n):
    from tf_geometric_amd.plan import CsrPlan
    ei = ei.clone()
    plan, flip = CsrPlan.build(ei, n, n), CsrPlan.build(torch.stack([ei[1], ei[0]]), n, n)
    return [plan.row_ptr, plan.col, plan.perm], [flip.row_ptr, flip.col, flip.perm]


# ---- 1. the layout equals the mirror, exactly ----------------------------------------------------------------------------------
def _one_hot(rng, n_cap, K):
    c = rng.integers(0, K, n_cap)
    S = np.zeros((n_cap, K), np.float32)
    S[np.arange(n_cap), c] = 1.0
    return S, c


def _integer_blocks(batch, c, K):
    """S^T A S for a one-hot S (cluster c[row]) and unit weights, from the batch's own live edges: integer-valued, so its zero
    pattern is the same in any precision."""
    B = batch.num_slots
    ei, egi = batch.edge_index.cpu().numpy(), batch.edge_graph_index.cpu().numpy()
    live = egi < B
    P = np.zeros((B * K, K), np.float32)
    np.add.at(P, (egi[live] * K + c[ei[0, live]], c[ei[1, live]]), 1.0)
    return P


def _check_layout(tfg, pooled, parent, P, K, drop, what):
    from tf_geometric_amd.plan import CACHE_KEY_PLAN, attached_plan
    from tf_geometric_amd.nn.pool.common_pool import CACHE_KEY_GRAPH_PLAN, _graph_plan
    B, cap = parent.num_slots, pooled.capacities
    assert cap == parent.dense_pooled_capacities(K, drop_diagonal=drop) and isinstance(pooled, tfg.data.StaticBatchGraph)
    assert (pooled.num_nodes, pooled.num_edges, pooled.num_graphs) == (cap.n_cap, cap.e_cap, B + 1)
    m = mirror_dense_pool_static(P, parent.graph_mask.cpu().numpy(), parent.counts.cpu().numpy(), K, drop, cap.n_cap, cap.e_cap,
                                 cap.sinks, cap.sink_degree)
    for key in ("edge_index", "node_graph_index", "edge_graph_index", "node_index", "edge_src", "counts"):
        _eq(getattr(pooled, key), m[key], "{}: {}".format(what, key))
    _eq(pooled.graph_row_ptr, m["pooled_row_ptr"], what + ": graph_row_ptr")
    _eq(pooled.edge_weight.detach(), mirror_pooled_weight(P, m["edge_src"]), what + ": edge_weight")
    assert pooled.y is parent.y and pooled.ids is parent.ids and pooled.graph_mask is parent.graph_mask
    assert pooled.check() is pooled
    plan = attached_plan(pooled.edge_index)
    assert plan is not None and plan is pooled.cache[CACHE_KEY_PLAN] and plan._transposed._transposed is plan
    _plan_eq(plan, m["plan"], what + ": by row")
    _plan_eq(plan._transposed, m["plan_t"], what + ": by column")
    rebuilt, flip = _rebuilt(pooled.edge_index, cap.n_cap)
    _plan_eq(plan, rebuilt, what + ": rebuilt")
    _plan_eq(plan._transposed, flip, what + ": rebuilt flip")
    ngi, version, graph_plan = pooled.cache[CACHE_KEY_GRAPH_PLAN]
    assert ngi is pooled.node_graph_index and version == ngi._version
    fresh = _graph_plan(ngi.clone(), B + 1, cap.n_cap, None)
    _plan_eq(graph_plan, [fresh.row_ptr, fresh.col, fresh.perm], what + ": graph plan")
    return m


@pytest.mark.parametrize("sink_degree", [1, 32])
@pytest.mark.parametrize("K", [1, 3, 20, 64])
def test_layout_equals_the_mirror_and_rebuilt_plans(tfg, K, sink_degree):
    store, _ = _world()
    rng = np.random.Generator(np.random.PCG64(5 * K + sink_degree))
    for name, ids in BATCHES.items():
        cap = store.static_capacities(len(ids), sink_degree=sink_degree)
        for drop in (False, True):
            batch = store.collate_static(_ids(ids), cap)
            S, c = _one_hot(rng, cap.n_cap, K)
            P = _integer_blocks(batch, c, K)
            ones = torch.ones(cap.e_cap, device=DEV)
            St = torch.from_numpy(S).to(DEV)
            if drop:
                pooled = tfg.nn.min_cut_pool_coarsen_static(batch.x, batch, St, normed_edge_weight=ones)
            else:
                batch.edge_weight = ones
                pooled = tfg.nn.diff_pool_coarsen_static(batch.x, batch, St)
            what = "K={} d={} {} drop={}".format(K, sink_degree, name, drop)
            m = _check_layout(tfg, pooled, batch, P, K, drop, what)
            if K == 1 and drop:
                assert pooled.capacities.e_cap == 0 and m["e_live"] == 0
            # a graph without nodes and a graph without edges own K rows and no edge; pooled x is S^T x, dead rows exactly 0
            live = [j for j, i in enumerate(ids) if i >= 0]
            for j, i in enumerate(ids):
                if i in (EMPTY, NO_EDGES):
                    assert not (m["edge_graph_index"] == j).any() and (m["node_graph_index"] == j).sum() == K
            x = batch.x.cpu().numpy().astype(np.float64)
            ngi = batch.node_graph_index.cpu().numpy()
            ref = np.zeros((cap.batch_size * K, F))
            rows = ngi < cap.batch_size
            np.add.at(ref, ngi[rows] * K + c[rows], x[rows])
            got = pooled.x.cpu().numpy()
            assert not got[m["m_live"]:].any() and m["m_live"] == K * len(live)
            # a float32 chain of at most 40 terms: |error| <= 40 * 2^-24 * sum |x| per entry
            bound = np.zeros_like(ref)
            np.add.at(bound, ngi[rows] * K + c[rows], np.abs(x[rows]))
            at = m["node_index"][:m["m_live"]]
            assert (np.abs(got[:m["m_live"]] - ref[at]) <= 40 * 2.0 ** -24 * bound[at]).all(), what + ": pooled x"


def _raw_kernel(P, mask, counts, K, drop, sink_degree):
    """tfgx_dense_pool_static on a P given as it is: a dict of its outputs (numpy), the capacities as the mirror takes them."""
    import ctypes
    from tf_geometric_amd import _lib as L
    from densepool_static_mirror import mirror_dense_capacities
    lib = L.require_gpu()
    B = len(mask)
    _, _, sinks, n_cap, e_cap = mirror_dense_capacities(B, K, sink_degree, drop)
    i32 = dict(dtype=torch.int32, device=DEV)
    Pt = torch.from_numpy(np.ascontiguousarray(P, np.float32)).to(DEV)
    mt, ct = torch.tensor(mask, dtype=torch.bool, device=DEV), torch.tensor(counts, **i32)
    out = dict(pooled_row_ptr=torch.full((B + 2,), -7, **i32), node_index=torch.full((n_cap,), -7, **i32),
               node_graph_index=torch.full((n_cap,), -7, **i32), node_map=torch.full((B * K,), -7, **i32),
               edge_index=torch.full((2, e_cap), -7, **i32), edge_src=torch.full((e_cap,), -7, **i32),
               edge_graph_index=torch.full((e_cap,), -7, **i32), counts=torch.full((4,), -7, **i32))
    plans, ios = [], []
    for _ in range(2):
        t = [torch.full((n_cap + 1,), -7, **i32), torch.full((e_cap,), -7, **i32), torch.full((e_cap,), -7, **i32)]
        io = L.CollatePlan()
        io.out_row_ptr, io.out_col, io.out_perm = (x.data_ptr() for x in t)
        plans.append(t)
        ios.append(io)
    ws = torch.empty(lib.tfgx_dense_pool_static_workspace_bytes(B), dtype=torch.uint8, device=DEV)
    a = L.DensePoolStaticArgs()
    a.P, a.ldp, a.graph_mask, a.parent_counts = Pt.data_ptr(), K, mt.data_ptr(), ct.data_ptr()
    a.B, a.K, a.drop_diagonal = B, K, int(drop)
    a.n_cap_out, a.e_cap, a.sinks, a.sink_degree = n_cap, e_cap, sinks, sink_degree
    a.pooled_row_ptr, a.node_index = out["pooled_row_ptr"].data_ptr(), out["node_index"].data_ptr()
    a.node_graph_index, a.node_map = out["node_graph_index"].data_ptr(), out["node_map"].data_ptr()
    a.out_row, a.out_col = out["edge_index"].data_ptr(), out["edge_index"].data_ptr() + 4 * e_cap
    a.out_edge_src, a.out_edge_graph_index = out["edge_src"].data_ptr(), out["edge_graph_index"].data_ptr()
    a.plan, a.plan_t = ctypes.pointer(ios[0]), ctypes.pointer(ios[1])
    a.counts, a.workspace, a.workspace_bytes = out["counts"].data_ptr(), ws.data_ptr(), int(ws.shape[0])
    L.check(lib.tfgx_dense_pool_static(ctypes.byref(a), L.stream_ptr()), "tfgx_dense_pool_static")
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["plan"], res["plan_t"] = ([x.cpu().numpy() for x in t] for t in plans)
    return res, (n_cap, e_cap, sinks)


@pytest.mark.parametrize("K,drop,sink_degree", [(3, False, 32), (3, True, 1), (64, False, 32), (1, True, 32), (20, True, 32)])
def test_kernel_on_signed_zeros_and_nans_equals_the_mirror(tfg, K, drop, sink_degree):
    """Every output of the launch sequence, the node_map included, on a P with -0.0 (no edge) and NaN (an edge) in live and in
    dead slots, more slots than one pass of a wave over the rows."""
    rng = np.random.Generator(np.random.PCG64(K))
    mask = [True, False, True, True, False, True]
    B = len(mask)
    P = (rng.integers(1, 5, (B * K, K)) * (rng.random((B * K, K)) < 0.5)).astype(np.float32)
    flat = P.reshape(-1)
    flat[rng.integers(0, flat.size, max(2, flat.size // 9))] = -0.0
    flat[rng.integers(0, flat.size, max(2, flat.size // 9))] = np.nan
    flat[0], flat[-1] = -0.0, np.nan                            # slot 0 (live) starts with -0.0, the last live slot ends with a NaN
    counts = [4, 11, 12, 2]
    got, (n_cap, e_cap, sinks) = _raw_kernel(P, mask, counts, K, drop, sink_degree)
    m = mirror_dense_pool_static(P, mask, counts, K, drop, n_cap, e_cap, sinks, sink_degree)
    for key in ("pooled_row_ptr", "node_index", "node_graph_index", "node_map", "edge_index", "edge_src", "edge_graph_index", "counts"):
        assert np.array_equal(got[key], m[key]), key
    for which in ("plan", "plan_t"):
        for a, b, part in zip(got[which], m[which], ("row_ptr", "col", "perm")):
            assert np.array_equal(a, b), (which, part)
    kept = flat[m["edge_src"][:m["e_live"]]]
    assert (np.isnan(kept) | (kept != 0)).all() and 0 not in m["edge_src"][:m["e_live"]]
    if not drop:
        assert np.isnan(kept).any() and flat.size - 1 in m["edge_src"]


# ---- 2. equals the eager route, bit for bit --------------------------------------------------------------------------------------
CROSSING = [5, 6, -1, NO_EDGES, 9, 2, -1, 10]          # 33 + 40 rows: the second graph crosses position 64, the fourth 128


@pytest.mark.parametrize("K", [3, 20])
def test_coarsening_equals_the_eager_route_bit_for_bit(tfg, K):
    from tf_geometric_amd import _lib as L
    store, d = _world()
    assert L.load_library().tfgx_seggram_block() == 64
    live = [i for i in CROSSING if i >= 0]
    starts = np.cumsum([0] + [SIZES[i][0] for i in live])
    assert any(a < 64 < b for a, b in zip(starts[:-1], starts[1:])), "no graph crosses a block boundary of the product"
    batch = store.collate_static(_ids(CROSSING))
    ref = store.collate(live)
    n_live, n_cap = ref.num_nodes, batch.capacities.n_cap
    gen = torch.Generator(device="cpu").manual_seed(K)
    S_live = torch.softmax(torch.randn((n_live, K), generator=gen) * 2.0, dim=-1).to(DEV)
    h_live = torch.randn((n_live, 6), generator=gen).to(DEV)
    S = torch.full((n_cap, K), 7.0, device=DEV)                 # what the dead rows hold must not matter
    h = torch.full((n_cap, 6), -3.0, device=DEV)
    S[:n_live], h[:n_live] = S_live, h_live
    slots = torch.tensor([j for j, i in enumerate(CROSSING) if i >= 0], dtype=torch.int32, device=DEV)
    G = len(live)
    for name, static_fn, eager_fn in (("diff_pool_coarsen", tfg.nn.diff_pool_coarsen_static, tfg.nn.diff_pool_coarsen),
                                      ("min_cut_pool_coarsen", tfg.nn.min_cut_pool_coarsen_static, tfg.nn.min_cut_pool_coarsen)):
        pooled = static_fn(h, batch, S)
        ex, eei, ew, engi = eager_fn(h_live, ref.edge_index, ref.edge_weight, ref.node_graph_index, S_live, num_graphs=G)
        m_live, e_live = int(pooled.counts[1]), int(pooled.counts[2])
        assert (m_live, e_live) == (G * K, int(eei.shape[1])) and int(pooled.counts[0]) == G
        assert torch.equal(pooled.x[:m_live], ex), name + ": pooled x"
        assert not pooled.x[m_live:].any(), name + ": dead rows of pooled x"
        assert torch.equal(pooled.edge_index[:, :e_live], eei), name + ": edge list"
        assert torch.equal(pooled.edge_weight[:e_live], ew), name + ": edge weights"
        assert torch.equal(pooled.node_graph_index[:m_live], slots[engi.long()]), name + ": node_graph_index"
        assert (pooled.edge_weight[e_live:] == 1.0).all() and (pooled.node_graph_index[m_live:] == len(CROSSING)).all()
        if name.startswith("min_cut"):
            assert (eei[0] != eei[1]).all() and e_live == (G - 1) * K * (K - 1)      # one graph without edges


# ---- 3. the two-level model against float64 -------------------------------------------------------------------------------------
UNITS = 8
CLUSTERS = (4, 2)
LIVE = [5, 3, NO_EDGES, 9, 4, 2, 10]
INTERLEAVED = [5, -1, 3, NO_EDGES, 9, -1, 4, 2, 10, -1]
NAMES = tuple("{}{} {}".format(w, level, p) for level in range(2) for w, p in
              (("pool", "bias"), ("feature", "kernel"), ("feature", "bias"), ("assign", "kernel"), ("assign", "bias"))) + \
    ("dense kernel", "dense bias")


def model_weights(num_classes, seed=11):
    """The weights of DenseModel as numpy float32, in the order of NAMES: kernels uniform in the Glorot range, biases away from
    zero so that they matter.  numpy alone, so that the conditions on the float64 reference can be looked at without a GPU."""
    rng = np.random.Generator(np.random.PCG64(seed))
    glorot = lambda a, b: (rng.uniform(-1, 1, (a, b)) * np.sqrt(6.0 / (a + b))).astype(np.float32)      # noqa: E731
    bias = lambda n: np.linspace(-0.2, 0.3, n).astype(np.float32)                                      # noqa: E731
    out = []
    for level, K in enumerate(CLUSTERS):
        f = F if level == 0 else UNITS
        out += [bias(UNITS), glorot(f, UNITS), bias(UNITS), glorot(f, K), bias(K)]
    return out + [glorot(2 * UNITS * len(CLUSTERS), num_classes), bias(num_classes)]


class DenseModel(object):
    """Two dense pooling levels (4 then 2 clusters; feature GNN GCN(8, relu), assignment GNN GCN(K)), mean || max readouts of the
    pooled batch after each, concatenated, then a dense layer.  kind "diff": DiffPool, the pooled weights tracked into level 2;
    "mincut": MinCutPool, the pooled weights detached, the two losses of both levels returned."""

    def __init__(self, tfg, kind, num_classes, seed=11):
        self.kind = kind
        weights = model_weights(num_classes, seed)
        cls = tfg.layers.DiffPool if kind == "diff" else tfg.layers.MinCutPool
        self.pools = []
        for level, K in enumerate(CLUSTERS):
            f = F if level == 0 else UNITS
            gnns = []
            for units, act in ((UNITS, tfg.relu), (K, None)):
                gcn = tfg.layers.GCN(units, activation=act)
                gcn._maybe_build([torch.empty(1, f)])
                gnns.append(gcn)
            pool = cls(gnns[0], gnns[1], UNITS, K, activation=torch.relu)
            pool.trainable(True)
            b, fk, fb, ak, ab = weights[5 * level:5 * level + 5]
            gnns[0].set_weights(kernel=fk, bias=fb)
            gnns[1].set_weights(kernel=ak, bias=ab)
            with torch.no_grad():
                pool.bias.copy_(torch.from_numpy(b))
            self.pools.append(pool)
        self.dense = tuple(torch.from_numpy(w).to(DEV).requires_grad_(True) for w in weights[-2:])

    def parameters(self):
        return [p for pool in self.pools for p in pool.parameters()] + list(self.dense)

    def __call__(self, batch, training=True, levels=None):
        from tf_geometric_amd import autograd as AG
        h, readouts, losses = batch.x, [], []
        for pool in self.pools:
            if self.kind == "diff":
                batch = pool.pool_static(h, batch, training=training)
            else:
                batch, (cut, orth) = pool.pool_static(h, batch, training=training, return_losses=True)
                losses += [cut, orth]
                batch.edge_weight = batch.edge_weight.detach()
            h = batch.x
            readouts.append(torch.cat([batch.readout(h, "mean"), batch.readout(h, "max")], dim=-1))
            if levels is not None:
                levels.append(batch)
        return AG.linear(torch.cat(readouts, dim=-1), *self.dense), losses


def _loss(model, batch, levels=None):
    logits, extra = model(batch, training=True, levels=levels)
    per_slot = torch.nn.functional.cross_entropy(logits, batch.y.reshape(-1), reduction="none")
    loss = torch.where(batch.graph_mask, per_slot, torch.zeros((), device=DEV)).sum() / batch.counts[0].clamp(min=1)
    for term in extra:
        loss = loss + term
    return logits, loss


def f64_model(d, live_ids, weights, kind):
    """Logits [len(live_ids), C] and the gradients of the objective wrt `weights` by float64 torch autograd, graph by graph on
    dense matrices — no edge list, no padding, no kernel of the package.  GCN: act(A_hat (x k) + b), A_hat = D^-1/2 (A + I) D^-1/2
    with D the row sums of A + I (nn/conv/gcn.py:32-130 defaults; duplicate edges add up).  A level: S = softmax(GCN_assign),
    P = S^T A S, x' = relu(S^T GCN_feature + bias); the next level's A is P (DiffPool), or P without its diagonal, detached,
    where this level's A was D^-1/2 A D^-1/2 first (MinCutPool, whose GNNs see the normalised A, with both losses of
    nn/pool/min_cut_pool.py:18-90 added to the objective).  Also returned: the smallest |pre-activation| of any ReLU, and the
    smallest |entry| of any S^T A S that is not structurally zero (a graph without edges, a dropped diagonal)."""
    leaves = [torch.from_numpy(np.asarray(w)).double().requires_grad_(True) for w in weights]
    margin, smallest = [np.inf], [np.inf]
    nb = len(live_ids)

    def gcn(A, h, k, b, relu):
        AI = A + torch.eye(A.shape[0], dtype=torch.float64)
        dis = AI.sum(dim=1).pow(-0.5)
        pre = (dis[:, None] * AI * dis[None, :]) @ (h @ k) + b
        if not relu:
            return pre
        if pre.numel():
            margin[0] = min(margin[0], float(pre.detach().abs().min()))
        return torch.relu(pre)

    rows, cuts, orths = [], [[], []], [[], []]
    for i in live_ids:
        n0, n1 = int(d["node_ptr"][i]), int(d["node_ptr"][i + 1])
        e0, e1 = int(d["edge_ptr"][i]), int(d["edge_ptr"][i + 1])
        n = n1 - n0
        A = torch.zeros((n, n), dtype=torch.float64)
        ei = torch.from_numpy(d["edge_index"][:, e0:e1].astype(np.int64)) - n0
        A.index_put_((ei[0], ei[1]), torch.from_numpy(d["edge_weight"][e0:e1]).double(), accumulate=True)
        h = torch.from_numpy(d["x"][n0:n1]).double()
        readouts = []
        for level, K in enumerate(CLUSTERS):
            bias, fk, fb, ak, ab = leaves[5 * level:5 * level + 5]
            if kind == "mincut":
                deg = A.sum(dim=1)
                dis = torch.where(deg > 0, deg.clamp(min=1e-300).pow(-0.5), torch.zeros_like(deg))
                A = dis[:, None] * A * dis[None, :]
            S = torch.softmax(gcn(A, h, ak, ab, False), dim=-1)
            hf = gcn(A, h, fk, fb, True)
            P = S.T @ A @ S
            structural = torch.zeros((K, K), dtype=torch.bool) if bool((A != 0).any()) else torch.ones((K, K), dtype=torch.bool)
            if kind == "mincut":
                structural = structural | torch.eye(K, dtype=torch.bool)
                cuts[level].append(-torch.trace(P) / (torch.trace(S.T @ (A.sum(dim=1)[:, None] * S)) + 1e-8))
                STS = S.T @ S
                dev = STS / (torch.sqrt((STS * STS).sum()) + 1e-8) - torch.eye(K, dtype=torch.float64) / np.sqrt(K)
                orths[level].append(torch.sqrt((dev * dev).sum()))
            if (~structural).any():
                smallest[0] = min(smallest[0], float(P.detach().abs()[~structural].min()))
            pre = S.T @ hf + bias
            margin[0] = min(margin[0], float(pre.detach().abs().min()))
            h = torch.relu(pre)
            A = P if kind == "diff" else (P * (1.0 - torch.eye(K, dtype=torch.float64))).detach()
            readouts.append(torch.cat([h.sum(dim=0) / (K + 1e-8), h.max(dim=0).values]))
        rows.append(torch.cat(readouts))
    logits = torch.stack(rows) @ leaves[-2] + leaves[-1]
    y = torch.from_numpy(np.asarray(d["y"]).reshape(-1)[np.asarray(live_ids)].astype(np.int64))
    loss = torch.nn.functional.cross_entropy(logits, y)
    if kind == "mincut":
        for level in range(len(CLUSTERS)):
            loss = loss + torch.stack(cuts[level]).sum() / nb + torch.stack(orths[level]).sum() / nb
    loss.backward()
    return logits.detach().numpy(), [p.grad.numpy() for p in leaves], margin[0], smallest[0]


@pytest.mark.parametrize("kind", ["diff", "mincut"])
def test_two_level_model_equals_float64_and_padding_is_inert(tfg, kind):
    """Logits of the live slots and every parameter gradient against float64 autograd on the live graphs (every entry within 1e-5
    of the tensor's largest reference magnitude), for the batch of the live slots alone, with dead slots appended and with dead
    slots interleaved; the three are asserted IDENTICAL, bit for bit.  The one exception is DESIGN.md §2.26's: the dense
    kernel gradient is a GEMM over the slots, which dead slots in the middle re-associate; there it is held to the float64
    bar and the difference printed.  The conditions on the inputs are asserted on the float64 reference."""
    assert [i for i in INTERLEAVED if i >= 0] == LIVE
    store, d = _world()
    C = 3
    model = DenseModel(tfg, kind, C)
    params = model.parameters()
    assert [tuple(p.shape) for p in params] == [tuple(w.shape) for w in model_weights(C)] and len(params) == len(NAMES)
    ref = f64_model(d, LIVE, model_weights(C), kind)
    print("float64 reference: smallest |pre-activation| = {:.3e}, smallest |entry| of S^T A S = {:.3e}".format(ref[2], ref[3]))
    assert ref[2] > 1e-5, "a ReLU of the float64 reference sits on its kink: choose other ids"
    assert ref[3] > 1e-6, "an entry of the float64 S^T A S is too small for its edge to be certain: choose other ids"
    worst = store.static_capacities(len(INTERLEAVED))
    results = {}
    for name, slots in (("live slots alone", LIVE), ("dead slots last", LIVE + [-1, -1, -1]), ("dead slots interleaved", INTERLEAVED)):
        cap = store.static_capacities(len(slots), max_nodes=worst.max_nodes, max_edges=worst.max_edges, sink_degree=worst.sink_degree)
        batch = store.collate_static(_ids(slots), cap)
        for p in params:
            p.grad = None
        levels = []
        logits, loss = _loss(model, batch, levels)
        loss.backward()
        live = batch.graph_mask
        assert live.tolist() == [i >= 0 for i in slots] and all(int(b.counts[3]) == 0 for b in levels)
        if kind == "diff":
            assert levels[0].edge_weight.requires_grad                 # the pooled weights train through level 2
        got_logits = logits.detach()[live].cpu().numpy()
        grads = [p.grad.detach().cpu().numpy().copy() for p in params]
        _close(got_logits, ref[0], name + ": logits")
        for g, r, what in zip(grads, ref[1], NAMES):
            assert np.isfinite(g).all(), what
            _close(g, r, "{}: d/d{}".format(name, what))
        for b in levels:                                               # dead pooled rows are exactly zero on every level
            assert not b.x.detach()[int(b.counts[1]):].any()
        assert torch.isfinite(logits).all()
        results[name] = (got_logits, grads, [b.edge_index[:, :int(b.counts[2])].cpu().numpy() for b in levels])
    alone_logits, alone_grads, alone_edges = results["live slots alone"]
    for name in ("dead slots last", "dead slots interleaved"):
        got_logits, grads, edges = results[name]
        assert all(np.array_equal(a, b) for a, b in zip(edges, alone_edges)), name + ": other pooled edges"
        equal = [np.array_equal(a, b) for a, b in zip(grads, alone_grads)]
        print("{}: logits identical: {}  gradients identical: {}".format(name, np.array_equal(got_logits, alone_logits),
                                                                        dict(zip(NAMES, equal))))
        assert np.array_equal(got_logits, alone_logits), name + ": logits differ from the batch without dead slots"
        for what, same, a, b in zip(NAMES, equal, grads, alone_grads):
            if what == "dense kernel" and name == "dead slots interleaved":
                print("{}: d/d{} max|difference| = {:.3e}".format(name, what, float(np.abs(a - b).max())))
                continue                                               # re-associated by the slot positions; held to float64 above
            assert same, "{}: d/d{} differs from the batch without dead slots".format(name, what)


# ---- 4. the MinCut losses --------------------------------------------------------------------------------------------------------
def test_min_cut_losses_equal_the_eager_route_and_dead_batches_give_zero(tfg):
    store, _ = _world()
    K = 3
    slots = [5, -1, 3, NO_EDGES, 9, -1]
    live = [i for i in slots if i >= 0]
    batch = store.collate_static(_ids(slots))
    ref = store.collate(live)
    n_live, n_cap = ref.num_nodes, batch.capacities.n_cap
    gen = torch.Generator(device="cpu").manual_seed(2)
    S_live = torch.softmax(torch.randn((n_live, K), generator=gen), dim=-1).to(DEV)
    S = torch.full((n_cap, K), 0.25, device=DEV)
    S[:n_live] = S_live
    S.requires_grad_(True)
    Se = S_live.clone().requires_grad_(True)
    cut, orth = tfg.nn.min_cut_pool_compute_losses_static(batch, S)
    (cut + orth).backward()
    ecut, eorth = tfg.nn.min_cut_pool_compute_losses(ref.edge_index, ref.edge_weight, ref.node_graph_index, Se, num_graphs=len(live))
    (ecut + eorth).backward()
    _close(cut.detach().cpu().numpy().reshape(1), ecut.detach().cpu().numpy().reshape(1), "cut_loss")
    _close(orth.detach().cpu().numpy().reshape(1), eorth.detach().cpu().numpy().reshape(1), "orth_loss")
    _close(S.grad[:n_live].cpu().numpy(), Se.grad.cpu().numpy(), "d/dS")
    assert not S.grad[n_live:].any(), "a dead row of S got a gradient"
    dead = store.collate_static(_ids([-1, -1, -1]))
    Sd = torch.full((dead.capacities.n_cap, K), 1.0 / K, device=DEV, requires_grad=True)
    cut, orth = tfg.nn.min_cut_pool_compute_losses_static(dead, Sd)
    (cut + orth).backward()
    assert float(cut.detach()) == 0.0 and float(orth.detach()) == 0.0 and torch.isfinite(Sd.grad).all()


# ---- 5. no host read, no sort ----------------------------------------------------------------------------------------------------
def _train_ids():
    return [i for i in range(len(SIZES)) if i != EMPTY]         # the orthogonality loss of a live graph without nodes has no derivative


def _train_store():
    if "train" not in _WORLD:
        import tf_geometric_amd as tfg
        sizes = [SIZES[i] for i in _train_ids()]
        d = random_dataset(np.random.Generator(np.random.PCG64(178)), sizes, F, y=False)
        d["y"] = (np.arange(len(sizes), dtype=np.int64) % 3).reshape(-1, 1)
        _WORLD["train"] = tfg.data.GraphStore.from_arrays(**d)
    return _WORLD["train"]


@pytest.mark.parametrize("kind", ["diff", "mincut"])
def test_ids_to_backward_makes_no_host_read_and_no_sort(tfg, monkeypatch, kind):
    from tf_geometric_amd.plan import CsrPlan
    store = _train_store()
    loader = store.static_loader(4, shuffle=True, seed=3)
    cap = store.static_capacities(4)
    model = DenseModel(tfg, kind, 3)

    def step():
        for p in model.parameters():
            p.grad = None
        batch = store.collate_static(loader.next_ids(), cap)
        levels = []
        loss = _loss(model, batch, levels)[1]
        loss.backward()
        return levels, loss

    step()                                                      # the warm call

    def no_build(*a, **k):
        raise AssertionError("a plan was built by sorting")

    monkeypatch.setattr(CsrPlan, "build", staticmethod(no_build))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        levels, loss = step()
        for b in levels:
            for op in ("mean", "sum", "max", "min"):
                b.readout(b.x.detach(), op)
            b.dense_pooled_capacities(2)
            b.pooled_capacities(ratio=0.5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert all(b.check() is b for b in levels)
    if kind == "diff":
        assert levels[0].edge_weight.requires_grad


# ---- 6. capture -------------------------------------------------------------------------------------------------------------------
def test_eager_dense_pools_still_refuse_a_capture(tfg, monkeypatch):
    store, _ = _world()
    b = store.collate([5, 3])
    gnn = tfg.layers.GCN(3)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="diff_pool cannot run inside a hipGraph capture"):
        tfg.nn.diff_pool(b.x, b.edge_index, b.edge_weight, b.node_graph_index, gnn, gnn, 3)
    with pytest.raises(RuntimeError, match="min_cut_pool cannot run inside a hipGraph capture"):
        tfg.nn.min_cut_pool(b.x, b.edge_index, b.edge_weight, b.node_graph_index, gnn, gnn, 3)


@pytest.mark.parametrize("kind", ["diff", "mincut"])
def test_pool_static_trains_under_a_capture(tfg, kind):
    store = _train_store()
    cap = store.static_capacities(4)

    def world():
        model = DenseModel(tfg, kind, 3, seed=21)
        opt = torch.optim.Adam(model.parameters(), lr=5e-3, capturable=True)
        loader = store.static_loader(4, shuffle=True, seed=13)
        return model, opt, loader, lambda: _loss(model, store.collate_static(loader.next_ids(), cap))[1]

    model, opt, loader, loss_fn = world()
    before = [p.detach().clone() for p in model.parameters()]
    step = tfg.CapturedTrainStep(loss_fn, opt)
    loader.cursor.zero_()                                       # the warm-up steps advanced it; the weights were rolled back
    captured = [float(step().detach()) for _ in range(3)]
    assert all(not torch.equal(a, b) for a, b in zip(before, model.parameters())), "a parameter was not trained"
    model_e, opt_e, loader_e, loss_fn_e = world()
    eager = []
    for _ in range(3):
        opt_e.zero_grad(set_to_none=True)
        loss = loss_fn_e()
        loss.backward()
        opt_e.step()
        eager.append(float(loss.detach()))
    print("eager    ", eager)
    print("captured ", captured, " bit-equal:", captured == eager)
    assert len(set(captured)) == 3                              # every replay trained on another batch, with other weights
    for c, e in zip(captured, eager):
        assert abs(c - e) <= 1e-6 * abs(e), (captured, eager)


# ---- 7. composition ---------------------------------------------------------------------------------------------------------------
def test_a_dense_pooled_batch_goes_through_the_other_static_pools(tfg):
    from tf_geometric_amd.plan import hub_policy
    from tf_geometric_amd.nn.pool.sort_pool_3d import convert_x_to_3d
    from tf_geometric_amd.utils.subgraph import pool_graph
    store, _ = _world()
    K = 5
    slots = [5, -1, 3, NO_EDGES, 9, -1, EMPTY]
    live = [i for i in slots if i >= 0]
    G = len(live)
    batch = store.collate_static(_ids(slots), store.static_capacities(len(slots), sink_degree=7))
    ref = store.collate(live)
    n_live, n_cap = ref.num_nodes, batch.capacities.n_cap
    gen = torch.Generator(device="cpu").manual_seed(4)
    S = torch.softmax(torch.randn((n_cap, K), generator=gen), dim=-1).to(DEV)
    pooled = tfg.nn.diff_pool_coarsen_static(batch.x, batch, S)
    ex, eei, ew, engi = tfg.nn.diff_pool_coarsen(ref.x, ref.edge_index, ref.edge_weight, ref.node_graph_index, S[:n_live].contiguous(),
                                                 num_graphs=G)
    cap = pooled.capacities
    m_live, e_live = int(pooled.counts[1]), int(pooled.counts[2])
    assert m_live == G * K and torch.equal(pooled.x[:m_live], ex) and torch.equal(pooled.edge_weight[:e_live], ew)
    slot_of = torch.tensor([j for j, i in enumerate(slots) if i >= 0], dtype=torch.int32, device=DEV)
    # the hub-rule metadata follows max(K, d), not the store's degrees
    assert pooled.max_degree() == K and batch.max_degree() == max(store._max_degrees())
    thr = hub_policy(cap.e_cap, cap.n_cap)[0]
    assert max(K, cap.sink_degree) <= thr
    for p in (pooled.cache["tfgx_csr_plan"], pooled.cache["tfgx_csr_plan"]._transposed):
        assert p._hub is False and p._row_order is False and p.hub_threshold == thr
    # (a) SAGPool at a fixed shape on the dense-pooled batch, against pool_graph on the eager pooled graph
    score = (torch.round(torch.randn(cap.n_cap, generator=gen) * 2.0) / 2.0).to(DEV).reshape(-1, 1)
    sag = tfg.nn.sag_pool_static(pooled.x, pooled, lambda inputs, training=None, cache=None: score, ratio=0.5,
                                 score_activation=torch.tanh)
    m2, e2 = int(sag.counts[1]), int(sag.counts[2])
    assert m2 == G * 3 and sag.max_degree() == K and sag.check() is sag          # ceil(5 / 2) of every live graph
    idx = sag.node_index[:m2].contiguous()
    px, pei, pw, pgi = pool_graph(ex, eei, ew, slot_of[engi.long()], idx, m_live, score=torch.tanh(score).reshape(-1)[:m_live])
    assert int(pei.shape[1]) == e2 and torch.equal(sag.x[:m2], px) and torch.equal(sag.edge_index[:, :e2], pei)
    assert torch.equal(sag.edge_weight[:e2], pw) and torch.equal(sag.node_graph_index[:m2], pgi) and not sag.x[m2:].any()
    for p in (sag.cache["tfgx_csr_plan"], sag.cache["tfgx_csr_plan"]._transposed):
        assert p._hub is False and p.hub_threshold == hub_policy(sag.capacities.e_cap, sag.capacities.n_cap)[0]
    rebuilt, flip = _rebuilt(sag.edge_index, sag.capacities.n_cap)
    _plan_eq(sag.cache["tfgx_csr_plan"], rebuilt, "sag of dense: rebuilt")
    _plan_eq(sag.cache["tfgx_csr_plan"]._transposed, flip, "sag of dense: rebuilt flip")
    # (b) to_3d: K rows per live slot, 3 of them taken
    got = pooled.to_3d(pooled.x, 3)
    want = convert_x_to_3d(ex, engi, k=3, num_sources=G)
    assert tuple(got.shape) == (len(slots), 3, F) and torch.equal(got[slot_of.long()], want)
    assert not got[[j for j, i in enumerate(slots) if i < 0]].any()
    # (c) a second dense level: same row positions in both routes, so bit for bit
    K2 = 2
    S2 = torch.softmax(torch.randn((cap.n_cap, K2), generator=gen), dim=-1).to(DEV)
    second = tfg.nn.diff_pool_coarsen_static(pooled.x, pooled, S2)
    sx, sei, sw, sngi = tfg.nn.diff_pool_coarsen(ex, eei, ew, engi, S2[:m_live].contiguous(), num_graphs=G)
    m3, e3 = int(second.counts[1]), int(second.counts[2])
    assert (m3, e3) == (G * K2, int(sei.shape[1])) and second.max_degree() == K2
    assert torch.equal(second.x[:m3], sx) and torch.equal(second.edge_index[:, :e3], sei) and torch.equal(second.edge_weight[:e3], sw)
    assert torch.equal(second.node_graph_index[:m3], slot_of[sngi.long()])
    assert second.capacities == pooled.dense_pooled_capacities(K2) and second.capacities.max_edges == len(slots) * 4
    for op in ("mean", "max"):
        r = second.readout(second.x, op)
        assert tuple(r.shape) == (len(slots), F) and not r[[j for j, i in enumerate(slots) if i < 0]].any()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_argument(tfg, monkeypatch):
    from tf_geometric_amd.data.graph_store import StaticBatchCapacities
    store, _ = _world()
    K = 3
    gnn = tfg.layers.GCN(K)

    def fresh():
        return store.collate_static(_ids([5, 3, -1, 4]))

    batch = fresh()
    n_cap = batch.capacities.n_cap
    S = torch.softmax(torch.randn((n_cap, K), device=DEV), dim=-1)
    plain = store.collate([5, 3])
    calls = {"diff_pool_coarsen_static": lambda x, b, s: tfg.nn.diff_pool_coarsen_static(x, b, s),
             "min_cut_pool_coarsen_static": lambda x, b, s: tfg.nn.min_cut_pool_coarsen_static(x, b, s),
             "min_cut_pool_compute_losses_static": lambda x, b, s: tfg.nn.min_cut_pool_compute_losses_static(b, s),
             "diff_pool_static": lambda x, b, s: tfg.nn.diff_pool_static(x, b, gnn, gnn, s.shape[1]),
             "min_cut_pool_static": lambda x, b, s: tfg.nn.min_cut_pool_static(x, b, gnn, gnn, s.shape[1])}
    for name, call in calls.items():
        with pytest.raises(ValueError, match=name + ": batch must be a StaticBatchGraph"):
            call(plain.x, plain, S)
        lost = fresh()
        lost.cache.clear()
        lost.edge_index = lost.edge_index.clone()
        with pytest.raises(ValueError, match=name + ": the batch has lost the plans"):
            call(lost.x, lost, S)
        other = fresh()
        other.capacities = StaticBatchCapacities(*((other.capacities.batch_size, other.capacities.max_nodes + 1) +
                                                   tuple(other.capacities[2:5]) + (n_cap + 1, other.capacities.e_cap)))
        with pytest.raises(ValueError, match=name + ": capacities .* do not describe the batch"):
            call(other.x, other, S)
    for name in ("diff_pool_coarsen_static", "min_cut_pool_coarsen_static", "min_cut_pool_compute_losses_static"):
        with pytest.raises(ValueError, match=r"{}: dense_assign must have one row per row of the batch \(\[{}, K\]\)".format(name, n_cap)):
            calls[name](batch.x, batch, S[:-1])
        for bad in (0, 65):
            with pytest.raises(ValueError, match=name + ": .*TFGX_SEGGRAM_MAX_K"):
                calls[name](batch.x, batch, torch.zeros((n_cap, bad), device=DEV))
    for name in ("diff_pool_coarsen_static", "min_cut_pool_coarsen_static", "diff_pool_static", "min_cut_pool_static"):
        with pytest.raises(ValueError, match=r"{}: x must have one row per row of the batch \(\[{}, F\]\)".format(name, n_cap)):
            calls[name](batch.x[:-1], batch, S)
    wide = tfg.layers.GCN(65)
    with pytest.raises(ValueError, match="diff_pool_static: .*TFGX_SEGGRAM_MAX_K"):
        tfg.nn.diff_pool_static(batch.x, batch, gnn, wide, 65)
    with pytest.raises(ValueError, match="diff_pool_static: num_clusters = 4 but dense_assign has 3 columns"):
        tfg.nn.diff_pool_static(batch.x, batch, gnn, gnn, 4)
    tracked = fresh()
    tracked.edge_weight = tracked.edge_weight.clone().requires_grad_(True)
    for name in ("min_cut_pool_coarsen_static", "min_cut_pool_compute_losses_static", "min_cut_pool_static"):
        with pytest.raises(NotImplementedError, match=name + ": an edge_weight that requires grad"):
            calls[name](tracked.x, tracked, S)
    tfg.nn.diff_pool_coarsen_static(tracked.x, tracked, S).edge_weight.sum().backward()       # DiffPool differentiates it
    assert tracked.edge_weight.grad is not None and torch.isfinite(tracked.edge_weight.grad).all()
    layer = tfg.layers.MinCutPool(gnn, gnn, None, K, use_bias=False)
    with pytest.raises(ValueError, match="return_loss_func and return_losses cannot be set"):
        layer.pool_static(batch.x, batch, return_loss_func=True, return_losses=True)
    with pytest.raises(ValueError, match="dense_pooled_capacities: num_clusters"):
        batch.dense_pooled_capacities(0)
    # host ids inside a capture; an identity array that would have to grow inside one
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="host graph ids inside a hipGraph capture"):
        tfg.nn.diff_pool_coarsen_static(batch.x, store.collate_static([5, 3, -1, 4]), S)
    monkeypatch.undo()
    small = tfg.data.GraphStore.from_arrays(**random_dataset(np.random.Generator(np.random.PCG64(9)), [(3, 4), (2, 1)], F))
    b = small.collate_static(_ids([0, 1, -1, -1]))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="longer identity array"):
        tfg.nn.diff_pool_coarsen_static(b.x, b, torch.full((b.capacities.n_cap, 64), 1.0 / 64, device=DEV))
    monkeypatch.undo()


# ---- 9. the examples ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demo", ["demo_diff_pool.py", "demo_min_cut_pool.py"])
@pytest.mark.parametrize("flags", [("--static", "--capture"), ()], ids=["capture", "default"])
def test_demos_run_and_end_with_a_finite_loss(demo, flags):
    """Each in a fresh child process: --static --capture at the sizes the feature's issue names, and the default invocation."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", demo)] + list(flags) +
                       ["--graphs", "60", "--steps", "6", "--batch-size", "8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("step")]
    print(r.stdout[-600:])
    assert lines and np.isfinite(float(lines[-1].split("loss")[1].split()[0])), r.stdout[-1500:]
    assert ("replayed" in r.stdout) == bool(flags)
