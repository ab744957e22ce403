# coding=utf-8
"""tfg.data.GraphStore.collate_static on the GPU (include/tfgx_collate_static.h): exact agreement with the numpy mirror of
tests/test_collate_static_abi.py on batches with dead slots that sit on the kernel's tile edges, the live part bit for bit what
collate gives, the three plans bit for bit against rebuilt (sorted) plans, overflow and bad ids, no host read from the ids to
the backward pass, a two-layer model against float64 autograd on the live graphs, the device-side loader, the capture of the
data side and of the whole training step, and the example."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_collate_static_abi import BAD_ID, OVERFLOW, mirror_collate_static
from test_gpu_collate import FS, LDS_OFFSETS, _eq, _plan_eq, _sizes, _store, _tile
from test_gpu_nbrblock import _close

pytestmark = pytest.mark.gpu

DEV = "cuda"
sys.path.insert(0, os.path.join(ROOT, "examples"))


def _args(d):
    return d["x"], d["edge_index"], d["edge_weight"], d["node_ptr"], d["edge_ptr"]


def _totals(ids):
    sizes = _sizes()
    live = [i for i in ids if 0 <= i < len(sizes)]
    return sum(sizes[i][0] for i in live), sum(sizes[i][1] for i in live)


def _batches(F):
    """name -> (ids, max_nodes, max_edges); None = the default (worst-case) capacity.  Graphs 0-8 are the special ones of
    tests/test_gpu_collate.py (0, 5: empty; 1, 2, 6: one node; 7: spans workgroups)."""
    tile = _tile()
    b = {"all slots live": (list(range(9, 21)), None, None),
         "dead first, in the middle and last": ([-1, 9, -1, -1, 10, 3, -1], None, None),
         "only dead slots": ([-1, -1, -1], None, None),
         "a graph three times": ([11, 11, 11], None, None),
         "empty graphs": ([0, 5, 9, 0, -1, 5], None, None),
         "the graph that spans workgroups": ([-1, 7, 12], None, None),
         "no slot": ([], None, None)}
    ids = [9, 10, -1, 11, 2]
    b["n_live == max_nodes exactly"] = (ids, _totals(ids)[0], None)
    b["e_live == max_edges exactly"] = (ids, None, _totals(ids)[1])
    # n_cap * F: the largest multiple of F up to tile - 1, and the smallest ones from tile and from tile + 1 on (F = 1: exactly
    # tile - 1, tile, tile + 1; F = 64: 960, 1024, 1088; F = 37: 999, 1036, 1036 — no multiple of 37 is AT the tile, so "at" and
    # "above" coincide there).  max_edges = 8 gives one sink at sink_degree 32 and 8 at sink_degree 1; max_nodes is what is left
    # of the rows (7 at the narrowest, F = 64 with sink_degree 1)
    small = [3, -1, 2, 1]                                       # 4 nodes, 6 edges
    for name, rows in (("below", (tile - 1) // F), ("at", -(-tile // F)), ("above", -(-(tile + 1) // F))):
        b["n_cap * F {} the tile".format(name)] = (small, ("rows", rows), 8)
    for off in (-1, 0, 1):
        b["e_cap = tile {:+d}".format(off)] = ([9, -1, 10, 11], None, tile + off)
    # B + 1 offsets: the last count that is searched in LDS and the first that is not, and well past it
    cycle = [0, 1, 2, 3, 4, 5, 6, -1, 9, 10, 11, 12]
    for B in (LDS_OFFSETS - 2, LDS_OFFSETS - 1, LDS_OFFSETS + 76):
        ids = [cycle[j % len(cycle)] for j in range(B)]
        n, e = _totals(ids)
        b["B + 1 = {}".format(B + 1)] = (ids, n + 5, e + 3)
    return b


def _capacities(store, name, ids, max_nodes, max_edges, sink_degree):
    if isinstance(max_nodes, tuple):                            # ("rows", n_cap): max_nodes = n_cap - P
        P = max(1, -(-max_edges // sink_degree))
        max_nodes = max_nodes[1] - P
        assert max_nodes >= _totals(ids)[0], "the case's own arithmetic: the live nodes fit beside the sinks"
    return store.static_capacities(len(ids), max_nodes=max_nodes, max_edges=max_edges, sink_degree=sink_degree)


def _ids_tensor(ids, dtype=torch.int32):
    return torch.tensor(ids, dtype=dtype, device=DEV)


def _check_against_mirror(batch, m, d, ids, what):
    for key in ("x", "edge_index", "edge_weight", "node_graph_index", "edge_graph_index"):
        assert getattr(batch, key).is_cuda
        _eq(getattr(batch, key), m[key], "{}: {}".format(what, key))
    _eq(batch.graph_mask, m["graph_mask"], what + ": graph_mask")
    _eq(batch.counts, m["counts"], what + ": counts")
    G = len(d["node_ptr"]) - 1
    _eq(batch.y, d["y"][np.clip(np.asarray(ids, dtype=np.int64), 0, G - 1)], what + ": y")


CASES = [(F, name, sd) for F in FS for name in _batches(F) for sd in (1, 32)]


# ---- 1. against the mirror, exactly; 2. the plans against rebuilt plans -------------------------------------------------------
@pytest.mark.parametrize("F,name,sink_degree", CASES, ids=lambda v: str(v).replace(" ", "_"))
def test_collate_static_equals_mirror_collate_and_rebuilt_plans(tfg, F, name, sink_degree):
    from tf_geometric_amd.plan import CsrPlan, CACHE_KEY_PLAN, attached_plan
    from tf_geometric_amd.nn.pool.common_pool import CACHE_KEY_GRAPH_PLAN, _graph_plan
    store, d = _store(F)
    ids, max_nodes, max_edges = _batches(F)[name]
    tile, B = _tile(), len(ids)
    cap = _capacities(store, name, ids, max_nodes, max_edges, sink_degree)
    m = mirror_collate_static(*_args(d), ids, max_nodes=cap.max_nodes, max_edges=cap.max_edges, sink_degree=sink_degree)
    n_cap, e_cap, n_live, e_live = cap.n_cap, cap.e_cap, m["n_live"], m["e_live"]
    assert (m["n_cap"], m["e_cap"], m["sinks"]) == (n_cap, e_cap, cap.sinks) and m["counts"][3] == 0
    if name.startswith("n_live =="):
        assert n_live == cap.max_nodes
    if name.startswith("e_live =="):
        assert e_live == cap.max_edges
    if name.startswith("n_cap * F"):
        assert n_cap * F in {1: (tile - 1, tile, tile + 1), 37: (999, 1036), 64: (960, 1024, 1088)}[F]
    if name.startswith("e_cap = tile"):
        assert e_cap == tile + int(name.split("tile")[1])
    batch = store.collate_static(_ids_tensor(ids, torch.int64 if B % 2 else torch.int32), cap)
    assert isinstance(batch, tfg.data.StaticBatchGraph) and isinstance(batch, tfg.BatchGraph)
    assert batch.num_graphs == B + 1 and (batch.num_nodes, batch.num_edges) == (n_cap, e_cap) and batch.capacities is cap
    what = "{} F={} sink_degree={}".format(name, F, sink_degree)
    _check_against_mirror(batch, m, d, ids, what)
    # the live part: bit for bit what collate gives for the live ids, once its positions are mapped to slots
    ref = store.collate(m["live_ids"])
    slots = torch.from_numpy(np.nonzero(m["graph_mask"])[0].astype(np.int32)).to(DEV)
    assert (ref.num_nodes, ref.num_edges) == (n_live, e_live)
    assert torch.equal(batch.x[:n_live], ref.x) and torch.equal(batch.edge_index[:, :e_live], ref.edge_index)
    assert torch.equal(batch.edge_weight[:e_live], ref.edge_weight)
    assert torch.equal(batch.node_graph_index[:n_live], slots[ref.node_graph_index.long()])
    assert torch.equal(batch.edge_graph_index[:e_live], slots[ref.edge_graph_index.long()])
    # the plans: attached, cached, transposed both ways, and what the mirror assembles
    plan = attached_plan(batch.edge_index)
    assert plan is not None and plan is batch.cache[CACHE_KEY_PLAN] and plan is CsrPlan.from_cache(batch.edge_index, n_cap, cache={})
    plan_t = plan.transposed()
    assert plan_t is plan._transposed and plan_t._transposed is plan and plan._edge_index is batch.edge_index
    assert (plan.n_dst, plan.n_src, plan.num_edges, plan_t.n_dst, plan_t.n_src, plan_t.num_edges) == (n_cap, n_cap, e_cap) * 2
    _plan_eq(plan, m["plan"], what + ": by destination")
    _plan_eq(plan_t, m["plan_t"], what + ": by source")
    ngi, version, graph_plan = batch.cache[CACHE_KEY_GRAPH_PLAN]
    assert ngi is batch.node_graph_index and version == ngi._version
    assert _graph_plan(ngi, B + 1, n_cap, batch.cache) is graph_plan                  # the readouts' lookup hits
    _plan_eq(graph_plan, m["graph_plan"], what + ": graph plan")
    # ... and what the library's own sort gives for the emitted list, for its flip and for node_graph_index with B + 1 graphs
    ei = batch.edge_index.clone()
    _plan_eq(plan, [getattr(CsrPlan.build(ei, n_cap, n_cap), k) for k in ("row_ptr", "col", "perm")], what + ": rebuilt")
    flip = CsrPlan.build(torch.stack([ei[1], ei[0]]), n_cap, n_cap)
    _plan_eq(plan_t, [flip.row_ptr, flip.col, flip.perm], what + ": rebuilt flip")
    fresh = _graph_plan(ngi.clone(), B + 1, n_cap, None)
    _plan_eq(graph_plan, [fresh.row_ptr, fresh.col, fresh.perm], what + ": rebuilt graph plan")
    assert (graph_plan.n_dst, graph_plan.n_src, graph_plan.num_edges) == (fresh.n_dst, fresh.n_src, fresh.num_edges)
    fresh_t, graph_t = fresh.transposed(), graph_plan.transposed()
    assert graph_t is graph_plan._transposed and graph_t._transposed is graph_plan
    _plan_eq(graph_t, [fresh_t.row_ptr, fresh_t.col, fresh_t.perm], what + ": rebuilt graph plan flip")
    assert (graph_t.n_dst, graph_t.n_src, graph_t.num_edges) == (fresh_t.n_dst, fresh_t.n_src, fresh_t.num_edges)


def test_plan_metadata_is_set_where_the_degrees_allow_it(tfg):
    """No row of a batch is longer than the dataset's largest degree or the sink degree: within the hub threshold both edge
    plans are marked (no hub lists, no walk order); beyond it they stay lazy."""
    from tf_geometric_amd.plan import hub_policy
    store, d = _store(37)
    degrees = store._max_degrees()
    assert degrees == (int(np.bincount(d["edge_index"][0]).max()), int(np.bincount(d["edge_index"][1]).max()))
    ids = _ids_tensor([9, 10, -1])
    for sink_degree, marked in ((32, max(degrees) <= 128), (4096, False)):
        cap = store.static_capacities(3, sink_degree=sink_degree)
        thr = hub_policy(cap.e_cap, cap.n_cap)[0]
        assert (max(max(degrees), sink_degree) <= thr) == marked
        plan = store.collate_static(ids, cap).cache["tfgx_csr_plan"]
        for p in (plan, plan._transposed):
            assert (p._hub is False and p._row_order is False and p.hub_threshold == thr) if marked else p._hub is None


# ---- 3. overflow and bad ids ----------------------------------------------------------------------------------------------------
def test_overflow_drops_a_suffix_and_bad_ids_are_dead_slots(tfg):
    store, d = _store(37)
    G = len(store)
    ids = [9, 10, -1, 11, 2, 12]
    sizes = _sizes()
    n2, e2 = _totals(ids[:2])
    for kw, first in ((dict(max_nodes=n2 + sizes[11][0] - 1), 3), (dict(max_edges=e2 + sizes[11][1] - 1), 3),
                      (dict(max_nodes=n2 + sizes[11][0] + 1, max_edges=10 ** 6), 5)):
        cap = store.static_capacities(len(ids), **kw)
        m = mirror_collate_static(*_args(d), ids, max_nodes=cap.max_nodes, max_edges=cap.max_edges)
        batch = store.collate_static(_ids_tensor(ids), cap)
        _check_against_mirror(batch, m, d, ids, "overflow {}".format(kw))
        assert m["counts"][3] == OVERFLOW and not m["graph_mask"][first:].any() and m["graph_mask"][:first].tolist() == [
            i >= 0 for i in ids[:first]]
        with pytest.raises(ValueError, match=r"slot {} \(graph {}\) and every later slot were dropped".format(first, ids[first])):
            batch.check()
    clean = store.collate_static(_ids_tensor(ids))
    assert clean.check() is clean and int(clean.counts[3]) == 0
    for bad_id, slot in ((G, 1), (G + 7, 4), (-2, 0)):
        bad = list(ids)
        bad.insert(slot, bad_id)
        cap = store.static_capacities(len(bad), max_nodes=clean.capacities.max_nodes, max_edges=clean.capacities.max_edges)
        batch = store.collate_static(_ids_tensor(bad, torch.int64), cap)
        m = mirror_collate_static(*_args(d), bad, max_nodes=cap.max_nodes, max_edges=cap.max_edges)
        _check_against_mirror(batch, m, d, bad, "bad id {}".format(bad_id))
        assert m["counts"][3] == BAD_ID and not m["graph_mask"][slot]
        # the other slots are as without it: the same rows and edges, the graph index moved past the dead slot
        n, e = int(clean.counts[1]), int(clean.counts[2])
        assert torch.equal(batch.x[:n], clean.x[:n]) and torch.equal(batch.edge_index[:, :e], clean.edge_index[:, :e])
        shifted = clean.node_graph_index[:n] + (clean.node_graph_index[:n] >= slot).to(torch.int32)
        assert torch.equal(batch.node_graph_index[:n], shifted)
        with pytest.raises(ValueError, match=r"graph id {} \(slot {} of the batch\) is outside \[0, {}\)".format(bad_id, slot, G)):
            batch.check()
    # an id beyond int32 is held to an out-of-range int32 on the device, and flagged like any other
    batch = store.collate_static(_ids_tensor([9, 1 << 40, -(1 << 40)], torch.int64))
    assert batch.graph_mask.tolist() == [True, False, False] and int(batch.counts[3]) == BAD_ID
    with pytest.raises(ValueError, match="capacities for 4 slots, 3 ids"):
        store.collate_static(_ids_tensor([9, 10, 11]), store.static_capacities(4))
    with pytest.raises(IndexError, match="int32 or int64"):
        store.collate_static(torch.zeros(3, device=DEV))


# ---- the model of the example ---------------------------------------------------------------------------------------------------
def _model(F, num_classes, seed=7):
    from demo_mean_pool import MeanPoolNetwork
    return MeanPoolNetwork(F, num_classes, seed=seed, drop_rate=0.0)


def _step(model, batch):
    from demo_mean_pool import batch_loss
    for p in model.parameters():
        p.grad = None
    loss = batch_loss(model, batch)
    loss.backward()
    return loss


# ---- 4. no host read --------------------------------------------------------------------------------------------------------------
def test_ids_to_backward_makes_no_host_read(tfg, monkeypatch):
    from tf_geometric_amd.plan import CsrPlan
    store, _ = _store(37)
    G = len(store)
    loader = store.static_loader(8, shuffle=True, seed=3)
    cap = store.static_capacities(8)
    model = _model(37, G)

    def step():
        batch = store.collate_static(loader.next_ids(), cap)
        return batch, _step(model, batch)

    step()                                                      # the warm call
    built = []
    real_build = CsrPlan.build

    def counting_build(edge_index, n_dst, n_src=None):
        built.append((int(n_dst), int(edge_index.shape[1])))
        return real_build(edge_index, n_dst, n_src)

    monkeypatch.setattr(CsrPlan, "build", staticmethod(counting_build))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batch, loss = step()
        for op in ("mean", "sum", "max", "min"):
            batch.readout(batch.x, op)
        with pytest.raises(RuntimeError):                       # collate is untouched: ids that live on the device synchronise
            store.collate(batch.ids.clamp(min=0))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert built == [], "plans were built: {}".format(built)
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    # check() is the one optional read
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            assert batch.check() is batch
    finally:
        torch.cuda.set_sync_debug_mode("default")
    reads = [w for w in seen if "synchroniz" in str(w.message)]
    assert len(reads) == 1, [str(w.message) for w in seen]


def test_host_ids_are_uploaded_when_eager_and_refused_inside_a_capture(tfg, monkeypatch):
    store, _ = _store(37)
    ids = [9, -1, 10]
    a, b = store.collate_static(ids), store.collate_static(_ids_tensor(ids))
    assert torch.equal(a.x, b.x) and torch.equal(a.edge_index, b.edge_index) and torch.equal(a.counts, b.counts)
    loader = store.static_loader(4)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="host graph ids inside a hipGraph capture"):
        store.collate_static(ids)
    with pytest.raises(RuntimeError, match="reshuffle uploads a host permutation"):
        loader.reshuffle(1)
    # capacities beyond the store's identity array: it is grown by an eager call, never inside a capture
    from test_collate_abi import random_dataset
    fresh = tfg.data.GraphStore.from_arrays(**random_dataset(np.random.Generator(np.random.PCG64(9)), [(3, 4), (2, 1)], 4))
    cap = fresh.static_capacities(4)
    assert cap.n_cap + 1 > int(fresh.node_ptr[-1]) + 1
    with pytest.raises(RuntimeError, match="longer identity array"):
        fresh.collate_static(_ids_tensor([0, 1, -1, -1]), cap)
    monkeypatch.undo()
    assert fresh.collate_static(_ids_tensor([0, 1, -1, -1]), cap).check().num_nodes == cap.n_cap


# ---- 5. model parity --------------------------------------------------------------------------------------------------------------
def _f64_model(store, live_ids, params, num_classes):
    """Logits [len(live_ids), C] and the parameter gradients of the mean cross-entropy, by float64 torch autograd on the
    BatchGraph.from_graphs batch of the live graphs: relu(A_hat (x K) + b) twice, A_hat = D^-1/2 (A + I) D^-1/2 with D the row
    sums of A + I (nn/conv/gcn.py:32-130 defaults), mean readout sum / (count + 1e-8), a dense layer.  Also the smallest
    |pre-activation| of the two ReLUs (the float64 reference's own distance from a kink)."""
    import tf_geometric_amd as tfg
    b = tfg.BatchGraph.from_graphs([store.graph(int(i)) for i in live_ids])
    n, nb = b.x.shape[0], len(live_ids)
    x = torch.from_numpy(b.x).double()
    row, col = torch.from_numpy(b.edge_index[0].astype(np.int64)), torch.from_numpy(b.edge_index[1].astype(np.int64))
    w = torch.from_numpy(b.edge_weight).double()
    ngi = torch.from_numpy(b.node_graph_index.astype(np.int64))
    y = torch.from_numpy(np.concatenate([np.asarray(g.y).reshape(-1) for g in b.graphs]).astype(np.int64))
    leaves = [p.detach().cpu().double().requires_grad_(True) for p in params]
    k0, b0, k1, b1, kd, bd = leaves
    dis = (torch.zeros(n, dtype=torch.float64).index_add_(0, row, w) + 1.0).pow(-0.5)
    what = dis[row] * w * dis[col]

    def layer(h, k, bias):
        h = h @ k
        pre = torch.zeros_like(h).index_add_(0, row, what[:, None] * h[col]) + (dis * dis)[:, None] * h + bias
        return torch.relu(pre), float(pre.detach().abs().min()) if pre.numel() else 1.0

    h, m0 = layer(x, k0, b0)
    h, m1 = layer(h, k1, b1)
    count = torch.zeros(nb, dtype=torch.float64).index_add_(0, ngi, torch.ones(n, dtype=torch.float64))
    pooled = torch.zeros((nb, h.shape[1]), dtype=torch.float64).index_add_(0, ngi, h) / (count[:, None] + 1e-8)
    logits = pooled @ kd + bd
    torch.nn.functional.cross_entropy(logits, y).backward()
    return logits.detach().numpy(), [p.grad.numpy() for p in leaves], min(m0, m1)


def test_two_layer_model_on_a_static_batch_equals_float64_on_the_live_graphs(tfg):
    """Logits of the live slots and every parameter gradient (loss masked) on static batches with dead slots — interleaved, and
    all at the end — and on the batch of the live slots alone, against float64 autograd on BatchGraph.from_graphs of the live
    graphs: every entry within 1e-5 of the tensor's largest reference magnitude.

    Padding is inert: the three batches are built at the SAME max_nodes / max_edges / sink_degree, so they differ in dead slots
    alone, and the logits of the live slots and the parameter gradients are asserted IDENTICAL, bit for bit, with and without
    them.  The one tensor for which that holds only when the dead slots come last is the dense layer's kernel gradient,
    pooled^T @ dlogits: it is a sum over the SLOTS, a dead slot adds an exact zero to it, and a dead slot in the middle moves the
    live terms to other places of the GEMM's blocked sum (tfgx_gemm_tn_f32), which re-associates the same terms.  There it is
    held to the float64 bar and the difference is printed."""
    from demo_mean_pool import batch_loss
    store, _ = _store(37)
    G = len(store)
    live_ids = [9, 3, 0, 10, 4, 2, 11]                          # an empty graph (0) among the live ones
    interleaved = [9, -1, 3, 0, 10, -1, 4, 2, 11, -1]
    assert [i for i in interleaved if i >= 0] == live_ids
    model = _model(37, G)
    params = model.parameters()
    names = ("k0", "b0", "k1", "b1", "dense kernel", "dense bias")
    assert [tuple(p.shape) for p in params] == [(37, 64), (64,), (64, 32), (32,), (32, G), (G,)]
    with torch.no_grad():
        for p in params:                                        # biases away from zero, so that they matter
            if p.dim() == 1:
                p.copy_(torch.linspace(-0.2, 0.3, p.numel(), device=DEV))
    ref_logits, ref_grads, margin = _f64_model(store, live_ids, params, G)
    print("float64 reference: smallest |pre-activation| = {:.3e}".format(margin))
    assert margin > 1e-5, "a ReLU of the float64 reference sits on its kink: choose other ids"
    worst = store.static_capacities(len(interleaved))
    results = {}
    for name, slots in (("live slots alone", live_ids), ("dead slots last", live_ids + [-1, -1, -1]),
                        ("dead slots interleaved", interleaved)):
        cap = store.static_capacities(len(slots), max_nodes=worst.max_nodes, max_edges=worst.max_edges, sink_degree=worst.sink_degree)
        assert (cap.n_cap, cap.e_cap, cap.sinks) == (worst.n_cap, worst.e_cap, worst.sinks)
        batch = store.collate_static(_ids_tensor(slots), cap)
        for p in params:
            p.grad = None
        logits = model(batch, training=True)
        y = batch.y.reshape(-1)
        per_slot = torch.nn.functional.cross_entropy(logits, y, reduction="none")
        loss = torch.where(batch.graph_mask, per_slot, torch.zeros((), device=DEV)).sum() / batch.counts[0].clamp(min=1)
        loss.backward()
        live = batch.graph_mask
        assert live.tolist() == [i >= 0 for i in slots]
        got_logits = logits.detach()[live].cpu().numpy()
        grads = [p.grad.detach().cpu().numpy().copy() for p in params]
        _close(got_logits, ref_logits, name + ": logits")
        for g, r, what in zip(grads, ref_grads, names):
            assert np.isfinite(g).all(), what
            _close(g, r, "{}: d/d{}".format(name, what))
        results[name] = (got_logits, grads)
        # the demo's loss is this loss
        assert torch.equal(batch_loss(model, batch).detach(), loss.detach())
        # readout rows of dead slots are exactly zero, for all four ops, and the live rows are the functional readouts'
        h = torch.randn((batch.num_nodes, 5), device=DEV)
        for op in ("mean", "sum", "max", "min"):
            r = batch.readout(h, op)
            assert tuple(r.shape) == (len(slots), 5) and not r[~live].any() and torch.isfinite(r).all()
            full = getattr(tfg.nn, op + "_pool")(h, batch.node_graph_index, batch.num_graphs)
            assert torch.equal(r[live], full[:len(slots)][live]), op
        with pytest.raises(ValueError, match="op must be one of"):
            batch.readout(h, "median")
    alone_logits, alone_grads = results["live slots alone"]
    for name in ("dead slots last", "dead slots interleaved"):
        got_logits, grads = results[name]
        equal = [np.array_equal(a, b) for a, b in zip(grads, alone_grads)]
        print("{}: logits identical: {}  gradients identical: {}".format(name, np.array_equal(got_logits, alone_logits),
                                                                        dict(zip(names, equal))))
        assert np.array_equal(got_logits, alone_logits), name + ": logits differ from the batch without dead slots"
        for what, same, a, b in zip(names, equal, grads, alone_grads):
            if what == "dense kernel" and name == "dead slots interleaved":
                print("{}: d/d{} max|difference| = {:.3e}".format(name, what, float(np.abs(a - b).max())))
                continue                                        # re-associated by the slot positions: the docstring; held to float64 above
            assert same, "{}: d/d{} differs from the batch without dead slots".format(name, what)


def test_readouts_take_the_cached_plan_and_match_the_rebuilt_one(tfg, monkeypatch):
    """mean / sum / max / min_pool and the readout layers with cache=: the plan the batch carries (collate and collate_static
    alike), bits equal to the sort-every-call route; without a cache they sort as before."""
    from tf_geometric_amd.plan import CsrPlan
    store, _ = _store(37)
    built = []
    real_build = CsrPlan.build

    def counting_build(edge_index, n_dst, n_src=None):
        built.append(int(n_dst))
        return real_build(edge_index, n_dst, n_src)

    monkeypatch.setattr(CsrPlan, "build", staticmethod(counting_build))
    for batch in (store.collate([9, 0, 10, 3]), store.collate_static(_ids_tensor([9, -1, 10, 3]))):
        h = torch.randn((batch.num_nodes, 7), device=DEV, requires_grad=True)
        for op, layer in (("mean", tfg.layers.MeanPool), ("sum", tfg.layers.SumPool), ("max", tfg.layers.MaxPool),
                          ("min", tfg.layers.MinPool)):
            func = getattr(tfg.nn, op + "_pool")
            del built[:]
            cached = func(h, batch.node_graph_index, batch.num_graphs, cache=batch.cache)
            by_layer = layer()([h, batch.node_graph_index, batch.num_graphs], cache=batch.cache)
            assert built == [], (op, built)
            sorted_ = func(h, batch.node_graph_index, batch.num_graphs)
            assert built == [batch.num_graphs], (op, built)
            # (the four slots: the dead graph of a static batch is one long row, which the sorted plan may cut into chunks)
            assert torch.equal(cached[:4], sorted_[:4]) and torch.equal(by_layer, cached), op
            ga, = torch.autograd.grad(cached.sum(), h)
            gb, = torch.autograd.grad(sorted_.sum(), h)
            assert torch.equal(ga, gb), op


# ---- 6. the loader ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("drop_last", [False, True])
def test_loader_hands_on_the_order_of_batches(tfg, shuffle, drop_last):
    store, _ = _store(1)
    G, B = len(store), 8
    assert G % B != 0

    def epoch(seed):
        return [b.y.reshape(-1).cpu().numpy() for b in store.batches(B, shuffle=shuffle, seed=seed, drop_last=drop_last)]

    loader = store.static_loader(B, shuffle=shuffle, seed=4, drop_last=drop_last)
    ref = epoch(4)
    assert loader.steps_per_epoch == len(ref) == (G // B if drop_last else G // B + 1)
    for chunk in ref + ref[:2]:                                 # one epoch, and the cursor wraps
        ids = loader.next_ids()
        assert ids.dtype == torch.int32 and ids.is_cuda and tuple(ids.shape) == (B,)
        ids = ids.cpu().numpy()
        assert np.array_equal(ids[:len(chunk)], chunk) and (ids[len(chunk):] == -1).all()
    assert int(loader.cursor) == (len(ref) + 2) * B
    order = loader.order
    assert loader.reshuffle(5) is loader and loader.order is order          # in place
    loader.cursor.zero_()
    for chunk in epoch(5):
        assert np.array_equal(loader.next_ids().cpu().numpy()[:len(chunk)], chunk)
    if shuffle:
        assert not np.array_equal(np.concatenate(epoch(5)), np.concatenate(ref))


# ---- 7. capture ---------------------------------------------------------------------------------------------------------------------
def _snapshot(batch):
    plan = batch.cache["tfgx_csr_plan"]
    graph_plan = batch.cache["tfgx_set2set_graph_plan"][2]
    ts = [batch.ids, batch.x, batch.edge_index, batch.edge_weight, batch.node_graph_index, batch.edge_graph_index, batch.y,
          batch.graph_mask, batch.counts, graph_plan.row_ptr]
    for p in (plan, plan._transposed):
        ts += [p.row_ptr, p.col, p.perm]
    return [t.clone() for t in ts]


def test_captured_ids_and_collate_yield_the_eager_batches(tfg):
    store, _ = _store(37)
    loader = store.static_loader(8, shuffle=True, seed=11)
    cap = store.static_capacities(8)
    store.collate_static(loader.next_ids(), cap)                # the warm call
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batch = store.collate_static(loader.next_ids(), cap)
    loader.cursor.zero_()
    replayed = []
    for _ in range(3):
        graph.replay()
        replayed.append(_snapshot(batch))
    assert int(loader.cursor) == 24
    loader.cursor.zero_()
    eager = [_snapshot(store.collate_static(loader.next_ids(), cap)) for _ in range(3)]
    for k, (r, e) in enumerate(zip(replayed, eager)):
        assert all(torch.equal(a, b) for a, b in zip(r, e)), "replay {}".format(k)
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[1][0], eager[2][0])


def test_captured_train_step_equals_eager_static_steps(tfg):
    from demo_mean_pool import make_static_loss_fn
    store, _ = _store(37)
    G = len(store)
    cap = store.static_capacities(8)

    def world():
        model = _model(37, G, seed=21)
        opt = torch.optim.Adam(model.parameters(), lr=5e-3, capturable=True)
        loader = store.static_loader(8, shuffle=True, seed=13)
        return model, opt, loader, make_static_loss_fn(model, store, loader, cap)

    model, opt, loader, loss_fn = world()
    step = tfg.CapturedTrainStep(loss_fn, opt)
    loader.cursor.zero_()                                       # the warm-up steps advanced it; the weights were rolled back
    captured = [float(step().detach()) for _ in range(3)]
    model_e, opt_e, loader_e, loss_fn_e = world()
    for a, b in zip(model.parameters(), model_e.parameters()):
        assert a.data_ptr() != b.data_ptr()
    eager = []
    for _ in range(3):
        opt_e.zero_grad(set_to_none=True)
        loss = loss_fn_e()
        loss.backward()
        opt_e.step()
        eager.append(float(loss.detach()))
    print("eager    ", eager)
    print("captured ", captured, " bit-equal:", captured == eager)
    _close(captured, eager, "captured vs eager losses")
    assert len(set(captured)) == 3                              # every replay trained on another batch, with other weights


# ---- 8. the example -----------------------------------------------------------------------------------------------------------------
def test_demo_mean_pool_static_capture_trains():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "demo_mean_pool.py"), "--static", "--capture", "--steps", "30"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(line.split("loss")[1].split()[0]) for line in r.stdout.splitlines() if line.startswith("step")]
    print(r.stdout[-600:])
    assert "collate_static, replayed" in r.stdout and len(losses) == 3 and losses[-1] < losses[0], r.stdout[-1500:]
