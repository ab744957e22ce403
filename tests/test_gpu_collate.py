# coding=utf-8
"""tfg.data.GraphStore.collate on the GPU (include/tfgx_collate.h): exact agreement with the numpy mirror of
tests/test_collate_abi.py on ragged batches that sit on the kernel's tile edges, its plans bit for bit against rebuilt (sorted)
plans, the hand-over to the layers (nothing is built for the input graph; bits equal to a host-built batch), no host
synchronisation, the refusals, the epoch iterator and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_collate_abi import mirror_collate, random_dataset

pytestmark = pytest.mark.gpu

DEV = "cuda"
FS = [1, 37, 64]              # scalar path with one float per row, scalar path with an odd row, the 16-byte vector path
LDS_OFFSETS = 1024            # tfgx_collate.hip kLdsOffsets: B + 1 offsets up to this many are searched in LDS, more in global memory


def _tile():
    from tf_geometric_amd import data
    return data.COLLATE_TILE


def _sizes():
    """(nodes, edges) of the dataset's graphs.  Ids 0-8 are the special ones the batches below name."""
    tile = _tile()
    rng = np.random.Generator(np.random.PCG64(5))
    special = [(0, 0),                         # 0: no nodes
               (1, 0),                         # 1: one node, no edge: the unit that fills n_out to an exact count
               (1, 1),                         # 2: one node with a self-loop: the unit that fills e_out
               (2, 5),                         # 3: two nodes, five edges: duplicates and self-loops for certain
               (17, 0),                        # 4: nodes without edges
               (0, 0),                         # 5: no nodes again
               (1, 3),                         # 6: one node, a triple self-loop
               (2 * tile // 2 + 76, 2 * tile + 3),     # 7: 1100 nodes (> tile / F for every F here), 2 tile + 3 edges
               (30, 0)]                        # 8
    assert special[7][0] > tile // min(FS) and special[7][1] == 2 * tile + 3
    rest = [(int(n), int(rng.integers(0, 3 * n))) for n in rng.integers(10, 51, 32)]
    return special + rest


_STORES = {}


def _store(F):
    """(GraphStore, its packed arrays) for feature width F: built once per width and left unchanged."""
    if F not in _STORES:
        import tf_geometric_amd as tfg
        d = random_dataset(np.random.Generator(np.random.PCG64(100 + F)), _sizes(), F, y=False)
        d["y"] = np.arange(len(_sizes()), dtype=np.int64).reshape(-1, 1)          # the label of a graph is its id
        _STORES[F] = (tfg.data.GraphStore.from_arrays(**d), d)
    return _STORES[F]


def _fill(target, unit_id, column):
    """Graph ids whose sizes in `column` (0 = nodes, 1 = edges) add up to exactly `target`: ordinary graphs while they fit, then
    the one-node unit graph `unit_id` (size 1 in that column)."""
    sizes = _sizes()
    ids, total = [], 0
    for g in range(9, len(sizes)):
        if total + sizes[g][column] > target:
            break
        ids.append(g)
        total += sizes[g][column]
    return ids + [unit_id] * (target - total)


def _batches(F):
    tile, G = _tile(), len(_sizes())
    b = {"one graph": [12], "the graph that spans workgroups": [7], "all graphs": list(range(G)), "reversed": list(range(G))[::-1],
         "the same graph three times": [11, 11, 11], "empty graphs first": [0, 5, 9, 10], "empty graphs last": [9, 10, 0, 5, 0],
         "two empty graphs in the middle": [9, 0, 5, 10, 3], "only empty graphs": [0, 5, 0], "no graph": [],
         "nodes but no edges": [4, 1, 8], "one-node graphs": [1, 2, 6, 2, 1]}
    for off in (-1, 0, 1):
        b["n_out = tile {:+d}".format(off)] = _fill(tile + off, 1, 0)
        b["e_out = tile {:+d}".format(off)] = _fill(tile + off, 2, 1)
    # n_out * F: the largest multiple of F up to tile - 1, and the smallest ones from tile and from tile + 1 on (F = 1: exactly
    # tile - 1, tile, tile + 1; F = 64: 960, 1024, 1088; F = 37: 999, 1036, 1036)
    for name, rows in (("below", (tile - 1) // F), ("at", -(-tile // F)), ("above", -(-(tile + 1) // F))):
        b["n_out * F {} the tile".format(name)] = _fill(rows, 1, 0)
    # B + 1 offsets: the last count that is searched in LDS and the first that is not, and well past it; graphs 0-6 and 9-12 in turn
    cycle = [0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12]
    for B in (LDS_OFFSETS - 1, LDS_OFFSETS, LDS_OFFSETS + 77):
        b["B = {}".format(B)] = [cycle[j % len(cycle)] for j in range(B)]
    return b


def _cases():
    return [(F, name) for F in FS for name in _batches(F)]


def _eq(t, ref, what):
    ref = ref.cpu() if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref))
    assert t.dtype == ref.dtype and tuple(t.shape) == tuple(ref.shape), "{}: {} {} vs {} {}".format(
        what, t.dtype, tuple(t.shape), ref.dtype, tuple(ref.shape))
    assert torch.equal(t.cpu(), ref), what


def _plan_eq(plan, ref, what):
    for name, r in zip(("row_ptr", "col", "perm"), ref):
        _eq(getattr(plan, name), r, "{} {}".format(what, name))


# ---- 1. against the mirror, exactly; 2. the plans against rebuilt plans -------------------------------------------------------
@pytest.mark.parametrize("F,name", _cases(), ids=lambda v: str(v).replace(" ", "_"))
def test_collate_equals_mirror_and_rebuilt_plans(tfg, F, name):
    from tf_geometric_amd.plan import CsrPlan, CACHE_KEY_PLAN, attached_plan
    from tf_geometric_amd.nn.pool.common_pool import CACHE_KEY_GRAPH_PLAN, _graph_plan
    store, d = _store(F)
    ids = _batches(F)[name]
    tile = _tile()
    m = mirror_collate(d["x"], d["edge_index"], d["edge_weight"], d["node_ptr"], d["edge_ptr"], ids)
    n_out, e_out = m["x"].shape[0], m["edge_index"].shape[1]
    if name.startswith("n_out = tile"):
        assert n_out == tile + int(name.split("tile")[1])
    if name.startswith("e_out = tile"):
        assert e_out == tile + int(name.split("tile")[1])
    if name.startswith("n_out * F"):
        assert n_out * F in {1: (tile - 1, tile, tile + 1), 37: (999, 1036), 64: (960, 1024, 1088)}[F]
    batch = store.collate(np.asarray(ids, dtype=np.int64) if len(ids) % 2 else ids)          # arrays and lists alike
    assert isinstance(batch, tfg.BatchGraph) and batch.num_graphs == len(ids)
    assert (batch.num_nodes, batch.num_edges) == (n_out, e_out)
    for key in ("x", "edge_index", "edge_weight", "node_graph_index", "edge_graph_index"):
        assert getattr(batch, key).is_cuda
        _eq(getattr(batch, key), m[key], "{} F={}: {}".format(name, F, key))
    _eq(batch.y, d["y"][np.asarray(ids, dtype=np.int64)], "y")
    # the plans: attached, cached, transposed both ways, and what the mirror's stable sorts give
    plan = attached_plan(batch.edge_index)
    assert plan is not None and plan is batch.cache[CACHE_KEY_PLAN] and plan is CsrPlan.from_cache(batch.edge_index, n_out, cache=batch.cache)
    assert plan is CsrPlan.from_cache(batch.edge_index, n_out, cache={})              # through the attachment alone
    plan_t = plan.transposed()
    assert plan_t is plan._transposed and plan_t._transposed is plan and plan._edge_index is batch.edge_index
    assert (plan.n_dst, plan.n_src, plan.num_edges, plan_t.n_dst, plan_t.n_src, plan_t.num_edges) == (n_out, n_out, e_out) * 2
    _plan_eq(plan, m["plan"], "by destination")
    _plan_eq(plan_t, m["plan_t"], "by source")
    ngi, version, graph_plan = batch.cache[CACHE_KEY_GRAPH_PLAN]
    assert ngi is batch.node_graph_index and version == ngi._version
    assert _graph_plan(ngi, len(ids), n_out, batch.cache) is graph_plan               # the readouts' lookup hits
    _plan_eq(graph_plan, m["graph_plan"], "graph plan")
    # ... and what the library's own sort gives for the emitted list, for its flip and for node_graph_index
    ei = batch.edge_index.clone()
    _plan_eq(plan, [getattr(CsrPlan.build(ei, n_out, n_out), k) for k in ("row_ptr", "col", "perm")], "rebuilt")
    flip = CsrPlan.build(torch.stack([ei[1], ei[0]]), n_out, n_out)
    _plan_eq(plan_t, [flip.row_ptr, flip.col, flip.perm], "rebuilt flip")
    if len(ids):
        fresh = _graph_plan(ngi.clone(), len(ids), n_out, None)
        _plan_eq(graph_plan, [fresh.row_ptr, fresh.col, fresh.perm], "rebuilt graph plan")
        assert (graph_plan.n_dst, graph_plan.n_src, graph_plan.num_edges) == (fresh.n_dst, fresh.n_src, fresh.num_edges)
        if n_out:
            fresh_t = fresh.transposed()
            _plan_eq(graph_plan.transposed(), [fresh_t.row_ptr, fresh_t.col, fresh_t.perm], "rebuilt graph plan flip")
            assert (graph_plan.transposed().n_dst, graph_plan.transposed().n_src) == (fresh_t.n_dst, fresh_t.n_src)


def test_two_calls_do_not_share_outputs(tfg):
    """The result is a pure function of the inputs, and a later batch leaves an earlier one alone."""
    store, _ = _store(37)
    a = store.collate([9, 10, 11])
    snapshot = [t.clone() for t in (a.x, a.edge_index, a.node_graph_index, a.cache["tfgx_csr_plan"].perm)]
    b = store.collate([12, 9])
    c = store.collate([9, 10, 11])
    for t, s, u in zip((a.x, a.edge_index, a.node_graph_index, a.cache["tfgx_csr_plan"].perm), snapshot,
                       (c.x, c.edge_index, c.node_graph_index, c.cache["tfgx_csr_plan"].perm)):
        assert torch.equal(t, s) and torch.equal(t, u) and t.data_ptr() != u.data_ptr()
    assert b.num_graphs == 2


# ---- 3. hand-over ---------------------------------------------------------------------------------------------------------------
def test_layers_build_nothing_for_a_collated_batch_and_match_a_host_built_one(tfg, monkeypatch):
    from tf_geometric_amd.plan import CsrPlan
    store, _ = _store(37)
    ids = [9, 3, 0, 10, 11, 4, 12, 13, 2, 14]
    gcn = tfg.layers.GCN(16, activation=tfg.relu, seed=1)
    pool = tfg.layers.SAGPool(score_gnn=tfg.layers.GCN(1, seed=2), ratio=0.5, score_activation=torch.tanh)
    gcn._maybe_build([torch.empty(1, 37)])
    pool.score_gnn._maybe_build([torch.empty(1, 16)])
    gcn.trainable(True)
    pool.trainable(True)
    params = gcn.parameters() + pool.parameters()
    gen = torch.Generator(device="cpu").manual_seed(3)
    gout = torch.randn((len(ids), 32), generator=gen).to(DEV)

    def run(batch, cache):
        for p in params:
            p.grad = None
        h = gcn([batch.x, batch.edge_index, batch.edge_weight], cache=cache, training=True)
        h, _, _, ngi = pool([h, batch.edge_index, batch.edge_weight, batch.node_graph_index], cache=cache, training=True)
        out = torch.cat([tfg.nn.mean_pool(h, ngi, batch.num_graphs), tfg.nn.max_pool(h, ngi, batch.num_graphs)], dim=-1)
        out.backward(gout)
        return out.detach().clone(), [p.grad.clone() for p in params]

    collated = store.collate(ids)
    host = tfg.BatchGraph.from_graphs([store.graph(i) for i in ids]).convert_data_to_tensor()
    assert torch.equal(host.x, collated.x) and torch.equal(host.edge_index, collated.edge_index)
    n_out, e_out = collated.num_nodes, collated.num_edges
    built = []
    real_build = CsrPlan.build

    def counting_build(edge_index, n_dst, n_src=None):
        built.append((int(n_dst), int(edge_index.shape[1])))
        return real_build(edge_index, n_dst, n_src)

    monkeypatch.setattr(CsrPlan, "build", staticmethod(counting_build))
    got = run(collated, collated.cache)
    # the input graph is the only one with n_out rows: the readouts sort the POOLED nodes by graph (n_dst = the graph count)
    assert [b for b in built if b[0] == n_out] == [], "plans were built for the collated graph: {}".format(built)
    del built[:]
    ref = run(host, {})
    assert len([b for b in built if b == (n_out, e_out)]) >= 2, built           # the forward plan and its flip, sorted
    assert torch.equal(got[0], ref[0]), "forward bits differ"
    assert all(g.abs().sum() > 0 for g in got[1])
    for a, b in zip(got[1], ref[1]):
        assert torch.equal(a, b), "parameter gradient bits differ"


# ---- 4. no host synchronisation -----------------------------------------------------------------------------------------------
def test_collate_does_not_synchronise(tfg):
    store, _ = _store(64)
    ids = [9, 10, 0, 11, 7]
    warm = store.collate(ids)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for form in (ids, np.asarray(ids), tuple(ids)):
            batch = store.collate(form)
        with pytest.raises(RuntimeError):                  # the documented exception: ids that live on the device
            store.collate(warm.y.reshape(-1))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(batch.x, warm.x) and torch.equal(batch.y, warm.y)
    from_device = store.collate(warm.y.reshape(-1))        # graph ids are the labels here
    assert torch.equal(from_device.edge_index, warm.edge_index)


# ---- 5. refusals, round trip, epochs ------------------------------------------------------------------------------------------
def test_refusals_and_round_trip(tfg):
    store, d = _store(37)
    G = len(store)
    for ids in ([G], [0, -1], np.asarray([3, G + 5])):
        with pytest.raises(IndexError, match="graph id"):
            store.collate(ids)
    graphs = [store.graph(i) for i in (3, 9)]
    with pytest.raises(ValueError, match="graph 2 has 5 features, graph 0 has 37"):
        tfg.data.GraphStore(graphs + [tfg.Graph(np.zeros((2, 5), np.float32), [[0], [1]], y=[[0]])])
    # Graph -> GraphStore -> graph(i): the arrays come back, in local ids
    again = tfg.data.GraphStore([store.graph(i) for i in range(G)])
    assert np.array_equal(again.node_ptr, d["node_ptr"]) and np.array_equal(again.edge_ptr, d["edge_ptr"])
    for i in (0, 3, 7, 20):
        a, b = again.graph(i), store.graph(i)
        n0, e0, e1 = d["node_ptr"][i], d["edge_ptr"][i], d["edge_ptr"][i + 1]
        assert np.array_equal(b.edge_index, d["edge_index"][:, e0:e1] - n0) and b.edge_index.dtype == np.int32
        for key in ("x", "edge_index", "edge_weight", "y"):
            assert np.array_equal(getattr(a, key), getattr(b, key)) and getattr(a, key).dtype == getattr(b, key).dtype, key
    # device graphs go in as well
    dev_store = tfg.data.GraphStore([g.convert_data_to_tensor() for g in graphs])
    assert torch.equal(dev_store.collate([1, 0]).x, store.collate([9, 3]).x)


def test_batches_cover_every_graph_once_and_follow_the_seed(tfg):
    store, _ = _store(1)
    G = len(store)

    def epoch(**kw):
        return [b.y.reshape(-1).cpu().numpy() for b in store.batches(8, **kw)]

    plain = epoch()
    assert [len(b) for b in plain] == [8] * (G // 8) + ([G % 8] if G % 8 else [])
    assert np.array_equal(np.concatenate(plain), np.arange(G))
    assert [len(b) for b in epoch(drop_last=True)] == [8] * (G // 8)
    a, b, c = epoch(shuffle=True, seed=4), epoch(shuffle=True, seed=4), epoch(shuffle=True, seed=5)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert not np.array_equal(np.concatenate(a), np.concatenate(c)) and not np.array_equal(np.concatenate(a), np.arange(G))
    assert sorted(np.concatenate(a)) == list(range(G)) and sorted(np.concatenate(c)) == list(range(G))
    with pytest.raises(ValueError):
        next(store.batches(0))


# ---- 6. example ---------------------------------------------------------------------------------------------------------------
def test_demo_graph_store_trains():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "demo_graph_store.py"), "--graphs", "600", "--epochs", "2",
                        "--batch-size", "64", "--lr", "0.002"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(line.split("loss")[1].split()[0]) for line in r.stdout.splitlines() if line.startswith("epoch")]
    assert "GraphStore.collate" in r.stdout and len(losses) == 2 and losses[1] < losses[0], r.stdout[-1500:]
