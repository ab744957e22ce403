# coding=utf-8
"""tfg.nn.sag_pool_static / topk_pool_static / SAGPool.pool_static on the GPU (include/tfgx_pool_static.h): the selection
against nn.topk_pool and the numpy mirror (tests/sagpool_static_mirror.py) on graphs that cross the wave, workgroup and LDS-cap
boundaries of the selection kernel; the pooled batch bit for bit against pool_graph on collate(live ids), the mirror and rebuilt
(sorted) plans, over two levels; a two-level model against float64 autograd; inert padding; no host read from the ids to the
backward pass; capture and replay of the whole training step; the refusals; the example."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from sagpool_static_mirror import CLAMPED, MAX_GRAPH_NODES, TOO_LONG, mirror_sag_pool_static, mirror_topk_static
from test_collate_abi import random_dataset
from test_collate_static_abi import mirror_collate_static
from test_gpu_collate import _eq, _plan_eq
from test_gpu_nbrblock import _close

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = 5
sys.path.insert(0, os.path.join(ROOT, "examples"))

# (nodes, edges): below / at / above one wave (64) and one workgroup (256), exactly the LDS cap, a graph without edges, an empty one
SIZES = [(0, 0), (1, 1), (2, 3), (3, 5), (7, 12), (33, 70), (64, 130), (65, 140), (256, 500), (257, 520), (6, 0),
         (MAX_GRAPH_NODES, 2 * MAX_GRAPH_NODES)]
BIG, NO_EDGES = 11, 10
BATCHES = {"B=1 the graph at the cap": [BIG],
           "B=1 dead": [-1],
           "B=4 all dead": [-1, -1, -1, -1],
           "B=4 small graphs": [NO_EDGES, 1, 2, 4],
           "B=9 dead first, in the middle and last, a graph twice": [-1, 7, 0, -1, 8, 9, 3, 3, -1],
           "B=9 every boundary": [5, 6, BIG, -1, 9, 8, 7, 4, NO_EDGES],
           # more slots than the 1024 threads of the table and scan workgroups: every thread owns more than one
           "B=1030 two slots a scan thread": [[10, 1, 2, 3, 4, -1][j % 6] for j in range(1030)]}
SELECTIONS = (dict(k=1), dict(k=3), dict(k=1000), dict(ratio=0.0), dict(ratio=0.3), dict(ratio=0.5), dict(ratio=1.0), dict(ratio=1.5))
_WORLD = {}


def _world():
    """(GraphStore, its packed arrays): built once and left unchanged."""
    if "w" not in _WORLD:
        import tf_geometric_amd as tfg
        d = random_dataset(np.random.Generator(np.random.PCG64(77)), SIZES, F, y=False)
        d["y"] = (np.arange(len(SIZES), dtype=np.int64) % 3).reshape(-1, 1)
        _WORLD["w"] = (tfg.data.GraphStore.from_arrays(**d), d)
    return _WORLD["w"]


def _train_store():
    """The graphs of the world that have nodes, the one at the cap left out: what the loaders of the training tests draw from
    (the max readout of a LIVE graph without nodes is float32 lowest — DESIGN.md §2.26 — and no level empties a graph: a graph
    of n >= 1 nodes keeps ceil(n / 2) >= 1)."""
    if "train" not in _WORLD:
        import tf_geometric_amd as tfg
        d = random_dataset(np.random.Generator(np.random.PCG64(78)), SIZES[1:BIG], F, y=False)
        d["y"] = (np.arange(BIG - 1, dtype=np.int64) % 3).reshape(-1, 1)
        _WORLD["train"] = tfg.data.GraphStore.from_arrays(**d)
    return _WORLD["train"]


def _args(d):
    return d["x"], d["edge_index"], d["edge_weight"], d["node_ptr"], d["edge_ptr"]


def _ids(ids):
    return torch.tensor(ids, dtype=torch.int32, device=DEV)


def _scores(rng, n_cap, n_live):
    """name -> float32 [n_cap]: many ties (halves), all equal, signed zeros among ties, one NaN."""
    ties = (np.round(rng.standard_normal(n_cap) * 2.0) / 2.0).astype(np.float32)
    zeros = rng.choice(np.asarray([-0.0, 0.0, 0.5, -0.5], np.float32), n_cap)
    nan = ties.copy()
    if n_live:
        nan[n_live // 2] = np.nan
    return {"ties": ties, "all equal": np.full(n_cap, 0.25, np.float32), "signed zeros": zeros, "one NaN": nan}


def _fixed(score):
    """A score "GNN" that returns a fixed device vector."""
    return lambda inputs, training=None, cache=None: score


# ---- 1. the selection -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BATCHES), ids=lambda v: v.replace(" ", "_"))
def test_selection_equals_topk_pool_and_the_mirror(tfg, name):
    store, d = _world()
    ids = BATCHES[name]
    B = len(ids)
    batch = store.collate_static(_ids(ids))
    cap = batch.capacities
    parent = mirror_collate_static(*_args(d), ids)
    n_live, n_cap = parent["n_live"], cap.n_cap
    rng = np.random.Generator(np.random.PCG64(3))
    for kind, score in _scores(rng, n_cap, n_live).items():
        s = torch.from_numpy(score).to(DEV)
        for kr in SELECTIONS:
            what = "{} / {} / {}".format(name, kind, kr)
            sel = tfg.nn.topk_pool_static(batch, s.reshape(-1, 1) if "k" in kr else s, **kr)
            pcap = batch.pooled_capacities(**kr)
            assert sel.capacities == pcap and tuple(sel.node_index.shape) == (pcap.n_cap,) and tuple(sel.node_map.shape) == (n_cap,)
            m = mirror_topk_static(parent["graph_plan"][0], score, B, cap.sinks, m_max=pcap.max_nodes, parent_counts=parent["counts"], **kr)
            m_live = m["m_live"]
            for key in ("node_index", "node_map", "pooled_row_ptr", "node_graph_index", "counts"):
                _eq(getattr(sel, key), m[key], what + ": " + key)
            assert int(sel.counts[3]) & (CLAMPED | TOO_LONG) == 0, what
            ref = tfg.nn.topk_pool(batch.node_graph_index[:n_live], s[:n_live], num_segments=B, **kr)
            assert torch.equal(sel.node_index[:m_live], ref), what + ": topk_pool"
            assert bool((sel.node_index[m_live:] == -1).all()), what


# ---- 2. the subgraph and the plans, over two levels ---------------------------------------------------------------------------------
def _check_level(tfg, store, pooled, m, parent_batch, score, scale, live_ref, what):
    """`pooled` against the mirror dict `m` (everything, the padded tail included), against rebuilt plans, and — where `live_ref`
    = (x, edge_index, edge_weight, node_graph_index -> slot) of the parent's live part is given — against pool_graph."""
    from tf_geometric_amd.plan import CsrPlan, CACHE_KEY_PLAN, attached_plan
    from tf_geometric_amd.nn.pool.common_pool import CACHE_KEY_GRAPH_PLAN, _graph_plan
    from tf_geometric_amd.utils.subgraph import induced_subgraph, pool_graph
    B, cap = pooled.num_slots, pooled.capacities
    n_out, e_cap, m_live, e_kept = cap.n_cap, cap.e_cap, m["n_live"], m["e_live"]
    assert isinstance(pooled, tfg.data.StaticBatchGraph) and pooled.num_graphs == B + 1
    assert (pooled.num_nodes, pooled.num_edges) == (n_out, e_cap) == (m["n_cap"], m["e_cap"])
    for key in ("x", "edge_index", "edge_weight", "node_graph_index", "edge_graph_index", "node_index", "edge_id", "counts"):
        _eq(getattr(pooled, key).detach(), m[key], "{}: {}".format(what, key))
    _eq(pooled.graph_row_ptr, m["pooled_row_ptr"], what + ": graph_row_ptr")
    assert pooled.y is parent_batch.y and pooled.ids is parent_batch.ids and pooled.graph_mask is parent_batch.graph_mask
    assert int(pooled.counts[3]) == 0 and pooled.check() is pooled
    plan = attached_plan(pooled.edge_index)
    assert plan is not None and plan is pooled.cache[CACHE_KEY_PLAN] and plan is CsrPlan.from_cache(pooled.edge_index, n_out, cache={})
    plan_t = plan.transposed()
    assert plan_t is plan._transposed and plan_t._transposed is plan and plan._edge_index is pooled.edge_index
    assert (plan.n_dst, plan.n_src, plan.num_edges, plan_t.n_dst, plan_t.n_src, plan_t.num_edges) == (n_out, n_out, e_cap) * 2
    _plan_eq(plan, m["plan"], what + ": by destination")
    _plan_eq(plan_t, m["plan_t"], what + ": by source")
    ei = pooled.edge_index.clone()
    _plan_eq(plan, [getattr(CsrPlan.build(ei, n_out, n_out), k) for k in ("row_ptr", "col", "perm")], what + ": rebuilt")
    flip = CsrPlan.build(torch.stack([ei[1], ei[0]]), n_out, n_out)
    _plan_eq(plan_t, [flip.row_ptr, flip.col, flip.perm], what + ": rebuilt flip")
    ngi, version, graph_plan = pooled.cache[CACHE_KEY_GRAPH_PLAN]
    assert ngi is pooled.node_graph_index and version == ngi._version
    assert _graph_plan(ngi, B + 1, n_out, pooled.cache) is graph_plan
    _plan_eq(graph_plan, m["graph_plan"], what + ": graph plan")
    fresh = _graph_plan(ngi.clone(), B + 1, n_out, None)
    _plan_eq(graph_plan, [fresh.row_ptr, fresh.col, fresh.perm], what + ": rebuilt graph plan")
    fresh_t = fresh.transposed()
    _plan_eq(graph_plan.transposed(), [fresh_t.row_ptr, fresh_t.col, fresh_t.perm], what + ": rebuilt graph plan flip")
    if live_ref is None or m_live == 0:
        return
    x, rei, rw, slot_of_node, n_live = live_ref
    idx = pooled.node_index[:m_live].contiguous()
    px, pei, pw, pgi = pool_graph(x, rei, rw, slot_of_node, idx, n_live, score=scale[:n_live])
    sub = induced_subgraph(rei, idx, n_live)
    assert int(pei.shape[1]) == e_kept
    assert torch.equal(pooled.x.detach()[:m_live], px) and torch.equal(pooled.edge_index[:, :e_kept], pei), what + ": pool_graph"
    assert torch.equal(pooled.edge_weight[:e_kept], pw) and torch.equal(pooled.node_graph_index[:m_live], pgi), what + ": pool_graph"
    assert torch.equal(pooled.edge_id[:e_kept], sub.edge_id) and torch.equal(pooled.edge_index[:, :e_kept], sub.edge_index)


@pytest.mark.parametrize("sink_degree", [1, 32])
@pytest.mark.parametrize("name", sorted(BATCHES), ids=lambda v: v.replace(" ", "_"))
def test_pooled_batch_equals_pool_graph_the_mirror_and_rebuilt_plans_over_two_levels(tfg, name, sink_degree):
    store, d = _world()
    ids = BATCHES[name]
    B = len(ids)
    cap = store.static_capacities(B, sink_degree=sink_degree)
    rng = np.random.Generator(np.random.PCG64(9))
    for kr in (dict(ratio=0.5), dict(k=3), dict(ratio=1.5)):
        batch = store.collate_static(_ids(ids), cap)
        parent = mirror_collate_static(*_args(d), ids, sink_degree=sink_degree)
        live_ids = parent["live_ids"]
        ref = store.collate(live_ids)
        slots = torch.from_numpy(np.nonzero(parent["graph_mask"])[0].astype(np.int32)).to(DEV)
        slot_of_node = slots[ref.node_graph_index.long()] if ref.num_nodes else ref.node_graph_index
        live_ref = (ref.x, ref.edge_index, ref.edge_weight, slot_of_node, ref.num_nodes)
        x_np = parent["x"]
        for level in range(2):
            n_cap = batch.capacities.n_cap
            score = (np.round(rng.standard_normal(n_cap) * 2.0) / 2.0).astype(np.float32)
            s = torch.from_numpy(score).to(DEV).reshape(-1, 1)
            scale = torch.tanh(s)
            x = batch.x.detach() if level else batch.x
            pooled = tfg.nn.sag_pool_static(x, batch, _fixed(s), score_activation=torch.tanh, **kr)
            m = mirror_sag_pool_static(parent, B, sink_degree, score, x=x_np, scale=scale.cpu().numpy(), **kr)
            what = "{} sink_degree={} {} level {}".format(name, sink_degree, kr, level)
            _check_level(tfg, store, pooled, m, batch, s, scale.reshape(-1), live_ref, what)
            # the next level pools this one: its live part is this level's live rows and kept edges
            m_live, e_kept = m["n_live"], m["e_live"]
            live_ref = (pooled.x.detach()[:m_live].contiguous(), pooled.edge_index[:, :e_kept].contiguous(),
                        pooled.edge_weight[:e_kept].contiguous(), pooled.node_graph_index[:m_live].contiguous(), m_live)
            batch, parent, x_np = pooled, m, m["x"]


def test_plan_metadata_follows_the_rule_of_collate_static(tfg):
    from tf_geometric_amd.plan import hub_policy
    store, _ = _world()
    batch = store.collate_static(_ids([5, 6, -1]))
    s = torch.randn(batch.capacities.n_cap, device=DEV)
    pooled = tfg.nn.sag_pool_static(batch.x, batch, _fixed(s), ratio=0.5)
    cap = pooled.capacities
    thr = hub_policy(cap.e_cap, cap.n_cap)[0]
    marked = max(max(store._max_degrees()), cap.sink_degree) <= thr
    plan = pooled.cache["tfgx_csr_plan"]
    for p in (plan, plan._transposed):
        assert (p._hub is False and p._row_order is False and p.hub_threshold == thr) if marked else p._hub is None
    graph_plan = pooled.cache["tfgx_set2set_graph_plan"][2]
    assert graph_plan._hub is False and graph_plan._transposed._hub is False


# ---- the two-level model ----------------------------------------------------------------------------------------------------------
class TwoLevelModel(object):
    """GCN(8, relu) -> pool_static(ratio 0.5, tanh) -> mean || max readout, twice, the readouts summed, then a dense layer."""

    def __init__(self, tfg, num_features, num_classes, seed=7):
        from demo_sag_pool_h import _glorot
        self.gcns, self.pools = [], []
        for level in range(2):
            self.gcns.append(tfg.layers.GCN(8, activation=tfg.relu, seed=seed + 2 * level))
            self.pools.append(tfg.layers.SAGPool(score_gnn=tfg.layers.GCN(1, seed=seed + 2 * level + 1), ratio=0.5,
                                                 score_activation=torch.tanh))
            self.gcns[-1]._maybe_build([torch.empty(1, num_features if level == 0 else 8)])
            self.pools[-1].score_gnn._maybe_build([torch.empty(1, 8)])
        for layer in self.gcns + self.pools:
            layer.trainable(True)
        gen = torch.Generator(device="cpu").manual_seed(seed + 100)
        self.dense = (_glorot(gen, 16, num_classes, torch.device(DEV)), torch.zeros(num_classes, device=DEV, requires_grad=True))

    def parameters(self):
        ps = []
        for gcn, pool in zip(self.gcns, self.pools):
            ps += gcn.parameters() + pool.parameters()
        return ps + list(self.dense)

    def __call__(self, batch, training=True, levels=None):
        from tf_geometric_amd import autograd as AG
        h, outputs = batch.x, []
        for gcn, pool in zip(self.gcns, self.pools):
            h = gcn([h, batch.edge_index, batch.edge_weight], cache=batch.cache, training=training)
            batch = pool.pool_static(h, batch, training=training)
            h = batch.x
            outputs.append(torch.cat([batch.readout(h, "mean"), batch.readout(h, "max")], dim=-1))
            if levels is not None:
                levels.append(batch)
        return AG.linear(outputs[0] + outputs[1], *self.dense)


def _loss(model, batch, levels=None):
    logits = model(batch, training=True, levels=levels)
    per_slot = torch.nn.functional.cross_entropy(logits, batch.y.reshape(-1), reduction="none")
    loss = torch.where(batch.graph_mask, per_slot, torch.zeros((), device=DEV)).sum() / batch.counts[0].clamp(min=1)
    return logits, loss


NAMES = ("gcn0 kernel", "gcn0 bias", "score0 kernel", "score0 bias", "gcn1 kernel", "gcn1 bias", "score1 kernel", "score1 bias",
         "dense kernel", "dense bias")


def _f64_model(store, live_ids, params, selections):
    """Logits [len(live_ids), C] and the parameter gradients of the mean cross-entropy by float64 torch autograd on
    BatchGraph.from_graphs of the live graphs.  GCN: act(A_hat (x K) + b), A_hat = D^-1/2 (A + I) D^-1/2 with D the row sums of
    A + I (nn/conv/gcn.py:32-130 defaults).  A level keeps the nodes `selections[level]` (the device's node_index: the float64
    side does not re-decide near-ties), scales them by tanh(score) and takes the induced subgraph (data/graph.py:276-359).
    Also the smallest |pre-activation| of the ReLUs."""
    import tf_geometric_amd as tfg
    b = tfg.BatchGraph.from_graphs([store.graph(int(i)) for i in live_ids])
    nb = len(live_ids)
    x = torch.from_numpy(b.x).double()
    row, col = torch.from_numpy(b.edge_index[0].astype(np.int64)), torch.from_numpy(b.edge_index[1].astype(np.int64))
    w = torch.from_numpy(b.edge_weight).double()
    ngi = torch.from_numpy(b.node_graph_index.astype(np.int64))
    y = torch.from_numpy(np.concatenate([np.asarray(g.y).reshape(-1) for g in b.graphs]).astype(np.int64))
    leaves = [p.detach().cpu().double().requires_grad_(True) for p in params]
    margin = [1.0]

    def gcn(h, k, bias, relu):
        n = h.shape[0]
        dis = (torch.zeros(n, dtype=torch.float64).index_add_(0, row, w) + 1.0).pow(-0.5)
        hk = h @ k
        pre = torch.zeros_like(hk).index_add_(0, row, (dis[row] * w * dis[col])[:, None] * hk[col]) + (dis * dis)[:, None] * hk + bias
        if not relu:
            return pre
        if pre.numel():
            margin[0] = min(margin[0], float(pre.detach().abs().min()))
        return torch.relu(pre)

    h, outputs = x, []
    for level in range(2):
        k, bias, sk, sb = leaves[4 * level:4 * level + 4]
        h = gcn(h, k, bias, True)
        score = gcn(h, sk, sb, False).reshape(-1)
        sel = torch.from_numpy(selections[level].astype(np.int64))
        node_map = torch.full((h.shape[0],), -1, dtype=torch.int64)
        node_map[sel] = torch.arange(sel.shape[0])
        h = h[sel] * torch.tanh(score[sel])[:, None]
        keep = (node_map[row] >= 0) & (node_map[col] >= 0)
        row, col, w, ngi = node_map[row[keep]], node_map[col[keep]], w[keep], ngi[sel]
        count = torch.zeros(nb, dtype=torch.float64).index_add_(0, ngi, torch.ones(h.shape[0], dtype=torch.float64))
        mean = torch.zeros((nb, h.shape[1]), dtype=torch.float64).index_add_(0, ngi, h) / (count[:, None] + 1e-8)
        mx = torch.stack([h[ngi == g].max(dim=0).values for g in range(nb)])
        outputs.append(torch.cat([mean, mx], dim=-1))
    logits = (outputs[0] + outputs[1]) @ leaves[8] + leaves[9]
    torch.nn.functional.cross_entropy(logits, y).backward()
    return logits.detach().numpy(), [p.grad.numpy() for p in leaves], margin[0]


LIVE = [5, 3, 6, 9, 4, 2, 7]            # no empty graph: the max readout of a live graph without nodes is float32 lowest
INTERLEAVED = [5, -1, 3, 6, 9, -1, 4, 2, 7, -1]


def _biased(model):
    with torch.no_grad():
        for p in model.parameters():                            # biases away from zero, so that they matter
            if p.dim() == 1:
                p.copy_(torch.linspace(-0.2, 0.3, p.numel(), device=DEV))
    return model


# ---- 3. features and gradients against float64; 4. the padding is inert ---------------------------------------------------------------
def test_two_level_model_equals_float64_and_padding_is_inert(tfg):
    """Logits of the live slots and every parameter gradient of the masked loss against float64 autograd on the live graphs
    (every entry within 1e-5 of the tensor's largest reference magnitude), for the batch of the live slots alone, with dead
    slots appended and with dead slots interleaved — at the SAME capacities, so the three differ in dead slots alone, and are
    asserted IDENTICAL, bit for bit.  The one exception is DESIGN.md §2.26's: the dense kernel gradient is a GEMM over the
    slots, which dead slots in the middle re-associate; there it is held to the float64 bar and the difference printed."""
    assert [i for i in INTERLEAVED if i >= 0] == LIVE
    store, _ = _world()
    C = 3
    model = _biased(TwoLevelModel(tfg, F, C))
    params = model.parameters()
    assert [tuple(p.shape) for p in params] == [(F, 8), (8,), (8, 1), (1,), (8, 8), (8,), (8, 1), (1,), (16, C), (C,)]
    worst = store.static_capacities(len(INTERLEAVED))
    results, ref = {}, None
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
        selections = [b.node_index[:int(b.counts[1])].cpu().numpy() for b in levels]
        if ref is None:
            ref = _f64_model(store, LIVE, params, selections)
            print("float64 reference: smallest |pre-activation| = {:.3e}".format(ref[2]))
            assert ref[2] > 1e-5, "a ReLU of the float64 reference sits on its kink: choose other ids"
        got_logits = logits.detach()[live].cpu().numpy()
        grads = [p.grad.detach().cpu().numpy().copy() for p in params]
        _close(got_logits, ref[0], name + ": logits")
        for g, r, what in zip(grads, ref[1], NAMES):
            assert np.isfinite(g).all(), what
            _close(g, r, "{}: d/d{}".format(name, what))
        # dead pooled rows are exactly zero on every level, and the logits of dead slots are finite
        for b in levels:
            assert not b.x.detach()[int(b.counts[1]):].any()
        assert torch.isfinite(logits).all()
        results[name] = (got_logits, grads, selections)
    alone_logits, alone_grads, alone_sel = results["live slots alone"]
    for name in ("dead slots last", "dead slots interleaved"):
        got_logits, grads, sel = results[name]
        assert all(np.array_equal(a, b) for a, b in zip(sel, alone_sel)), name + ": another selection"
        equal = [np.array_equal(a, b) for a, b in zip(grads, alone_grads)]
        print("{}: logits identical: {}  gradients identical: {}".format(name, np.array_equal(got_logits, alone_logits),
                                                                        dict(zip(NAMES, equal))))
        assert np.array_equal(got_logits, alone_logits), name + ": logits differ from the batch without dead slots"
        for what, same, a, b in zip(NAMES, equal, grads, alone_grads):
            if what == "dense kernel" and name == "dead slots interleaved":
                print("{}: d/d{} max|difference| = {:.3e}".format(name, what, float(np.abs(a - b).max())))
                continue                                        # re-associated by the slot positions; held to float64 above
            assert same, "{}: d/d{} differs from the batch without dead slots".format(name, what)


# ---- 5. no host read ------------------------------------------------------------------------------------------------------------------
def test_ids_to_backward_makes_no_host_read(tfg, monkeypatch):
    from tf_geometric_amd.plan import CsrPlan
    store = _train_store()
    loader = store.static_loader(4, shuffle=True, seed=3)
    cap = store.static_capacities(4)
    model = _biased(TwoLevelModel(tfg, F, 3))

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
            b.pooled_capacities(ratio=0.5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert all(b.check() is b for b in levels)


# ---- 6. capture -------------------------------------------------------------------------------------------------------------------------
def test_sag_pool_refuses_a_capture_and_pool_static_trains_under_one(tfg, monkeypatch):
    store, _ = _world()
    cap = store.static_capacities(4)
    batch = store.collate_static(_ids([5, 6, -1, 4]), cap)
    gnn = tfg.layers.GCN(1, seed=1)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="sag_pool cannot run inside a hipGraph capture"):
        tfg.nn.sag_pool(batch.x, batch.edge_index, batch.edge_weight, batch.node_graph_index, gnn, ratio=0.5)
    monkeypatch.undo()
    store = _train_store()
    cap = store.static_capacities(4)

    def world():
        model = _biased(TwoLevelModel(tfg, F, 3, seed=21))
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


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_argument(tfg, monkeypatch):
    store, d = _world()
    batch = store.collate_static(_ids([5, 6, -1, 4]))
    cap = batch.capacities
    s = torch.randn(cap.n_cap, device=DEV)
    gnn = _fixed(s)
    plain = store.collate([5, 6])
    with pytest.raises(ValueError, match="sag_pool_static: batch must be a StaticBatchGraph"):
        tfg.nn.sag_pool_static(plain.x, plain, gnn, ratio=0.5)
    with pytest.raises(ValueError, match="topk_pool_static: batch must be a StaticBatchGraph"):
        tfg.nn.topk_pool_static(plain, s, ratio=0.5)
    with pytest.raises(ValueError, match=r"sag_pool_static: x must have one row per row of the batch \(\[{}, F\]\)".format(cap.n_cap)):
        tfg.nn.sag_pool_static(batch.x[:-1], batch, gnn, ratio=0.5)
    with pytest.raises(ValueError, match="topk_pool_static: score must hold one value per row"):
        tfg.nn.topk_pool_static(batch, s[:-1], ratio=0.5)
    for kw, word in ((dict(), "got neither"), (dict(k=1, ratio=0.5), "not both"), (dict(k=-1), "k must be an integer"),
                     (dict(ratio=-1.0), "at least 0")):
        with pytest.raises(ValueError, match="pooled_capacities: .*" + word):
            tfg.nn.sag_pool_static(batch.x, batch, gnn, **kw)
    with pytest.raises(ValueError, match="sag_pool_static: capacities for 5 slots, the batch has 4"):
        tfg.nn.sag_pool_static(batch.x, batch, gnn, ratio=0.5, capacities=store.static_capacities(5))
    other = store.collate_static(_ids([5, 6, -1, 4]), store.static_capacities(4, sink_degree=7)).pooled_capacities(ratio=0.5)
    with pytest.raises(ValueError, match="sag_pool_static: capacities .* were made for other parent capacities"):
        tfg.nn.sag_pool_static(batch.x, batch, gnn, ratio=0.5, capacities=other)
    tracked = store.collate_static(_ids([5, 6, -1, 4]))
    tracked.edge_weight = tracked.edge_weight.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="sag_pool_static: edge_weight requires grad"):
        tfg.nn.sag_pool_static(tracked.x, tracked, gnn, ratio=0.5)
    layer = tfg.layers.SAGPool(score_gnn=gnn, ratio=0.5)
    with pytest.raises(ValueError, match="sag_pool_static: batch must be a StaticBatchGraph"):
        layer.pool_static(plain.x, plain)
    # a store with a graph one node above the LDS cap refuses the static pooling route by name, on the host
    big = random_dataset(np.random.Generator(np.random.PCG64(1)), [(3, 2), (MAX_GRAPH_NODES + 1, 4)], F)
    long_store = tfg.data.GraphStore.from_arrays(**big)
    long_batch = long_store.collate_static(_ids([0, -1]))
    with pytest.raises(ValueError, match="{} nodes, more than the {} the static pooling route".format(MAX_GRAPH_NODES + 1, MAX_GRAPH_NODES)):
        tfg.nn.sag_pool_static(long_batch.x, long_batch, _fixed(torch.zeros(long_batch.capacities.n_cap, device=DEV)), ratio=0.5)
    # capacities that were not made for this ratio: the kept nodes are cut off at them, flagged, and check() says so
    small = batch.pooled_capacities(k=1)                       # 4 kept nodes at the most; ratio 1.0 keeps all 104
    pooled = tfg.nn.sag_pool_static(batch.x, batch, gnn, ratio=1.0, capacities=small)
    assert int(pooled.counts[3]) == CLAMPED and int(pooled.counts[1]) == small.max_nodes
    with pytest.raises(ValueError, match="sag_pool_static: the kept nodes exceeded max_nodes = {}".format(small.max_nodes)):
        pooled.check()
    # inside a capture the store's identity array is not grown
    fresh = tfg.data.GraphStore.from_arrays(**random_dataset(np.random.Generator(np.random.PCG64(9)), [(3, 4), (2, 1)], F))
    b = fresh.collate_static(_ids([0, 1, -1, -1]))
    fresh._resident()["arange"] = fresh._resident()["arange"][:2]          # as if the store had never made a longer one
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="longer identity array"):
        tfg.nn.sag_pool_static(b.x, b, _fixed(torch.zeros(b.capacities.n_cap, device=DEV)), ratio=0.5)
    monkeypatch.undo()


def test_example_step_replayed_equals_eager_with_dropout_on(tfg):
    """examples/demo_sag_pool_h.make_static_step: the replayed step draws the batches AND the dropout masks of the eager static
    steps (the loader's cursor and the dropout generator are rolled back after the capture's warm-up), so with the model's
    dropout 0.5 ON four replays give the losses of four eager steps from the same weights — within 1e-6 of |loss|, the bound of
    the dropout-free comparison above."""
    import demo_sag_pool_h as demo
    data = demo.make_dataset(48, 3)
    store = demo.graph_store(data, range(48))
    cap = store.static_capacities(16)
    losses = {}
    for capture in (False, True):
        torch.manual_seed(5)
        model = demo.SAGPoolHModel(data.num_features, data.num_classes, seed=5)
        opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
        loader = store.static_loader(16, shuffle=True, seed=6)
        step = demo.make_static_step(model, store, loader, cap, opt, capture)
        losses[capture] = [float(step().detach()) for _ in range(4)]
        assert int(loader.cursor) == 64
    print("eager    ", losses[False])
    print("replayed ", losses[True], " bit-equal:", losses[True] == losses[False])
    assert len(set(losses[False])) == 4
    for c, e in zip(losses[True], losses[False]):
        assert abs(c - e) <= 1e-6 * abs(e), losses


# ---- 8. the example ---------------------------------------------------------------------------------------------------------------------
def test_demo_sag_pool_h_capture_trains():
    """The example under --capture at the sizes the feature's issue names: it runs and its loss falls.

    The margin is small and is what it is because the run is deterministic: per-epoch means of the 6 training losses (dropout
    0.5 on, lr = 5e-4, seed 0) were 0.692901 and 0.692636 in the recorded run, a trend of -3e-4 per epoch under single losses
    that scatter by 1.5e-3.  The replayed route gives exactly the losses of the eager --static route (the test above), whose
    first epoch is bit-equal to the default route's; before make_static_step rolled the dropout generator back after the
    capture's warm-up, the replay drew other masks and its two means were 0.6931384 and 0.6931391."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "demo_sag_pool_h.py"), "--capture", "--graphs", "200",
                        "--epochs", "2", "--batch-size", "32"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(line.split("loss")[1].split()[0]) for line in r.stdout.splitlines() if line.startswith("epoch")]
    print(r.stdout[-600:])
    assert "collate_static, replayed" in r.stdout and len(losses) == 2 and losses[1] < losses[0], r.stdout[-1500:]
