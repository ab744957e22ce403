# coding=utf-8
"""Fixed-shape minibatch sampling on the GPU (include/tfgx_nbrstatic.h, RandomNeighborSampler.sample_blocks_static).

The 401-node graph of tests/test_gpu_nbrblock.py serves the sampling tests (in-degrees 0 / 1 / 4-6 / 20 / 33 / 100, a hub of
5000, a sink id that only appears as a neighbour); its _model_world serves the model tests.

  1. A static minibatch IS sample_blocks of the live seeds: the same nodes, edges and weight bits under the rank-among-live
     mapping, the tail exactly the sink self-loops, every shape static_capacities', the whole equal to mirror_static_blocks.
  2. Both attached plans equal CsrPlan.build of the list and of the flipped list; forward and backward build no plan.
  3. No host read: sampling, gather and a two-layer forward report zero synchronising calls, check() one.
  4. gather / input_aggregate: exact zeros for dead rows, the dynamic route's bits for live ones, over widths and a strided view.
  5. Two layers over the static blocks, fused and unfused, meet the float64 bar; dead seeds contribute nothing.
  6. The relabel table is clean after every call; bad seeds are dead slots that check() reports.
  7. Capture: a captured sampler draws a fresh sample per replay; a captured training step equals the eager steps; seed=None
     is refused inside a capture.
"""
import warnings

import numpy as np
import pytest
import torch

from test_nbrstatic_abi import mirror_static_blocks
from test_gpu_nbrblock import (_graph, _mirror_of, HUB, ISOLATED, SINK, _model_world, _weights, _layers, _f64_model, _close)

pytestmark = pytest.mark.gpu

SEEDS = [HUB, 17, -1, ISOLATED, SINK, 7, -1, 399]
LIVE = [s for s in SEEDS if s >= 0]
CASES = [([5], False), ([5], True), ([5, 3], False), ([5, 3], True), ([40, 5, 2], False), ([40, 5, 2], True), ([3, 0], False),
         ([3, 0], True)]


@pytest.fixture(scope="module")
def world(tfg):
    ei, ew = _graph()
    dev = tfg._lib.device()
    ei_t, ew_t = torch.from_numpy(ei).to(dev), torch.from_numpy(ew).to(dev)
    return {"ei": ei_t, "ew": ew_t, "sampler": tfg.utils.RandomNeighborSampler(ei_t, ew_t), "full": {}, "dev": dev}


def _rank(live):
    """static virtual id -> its rank among the live ones (the dynamic virtual id)."""
    return (torch.cumsum(live.to(torch.int64), 0) - 1).to(torch.int32)


def _assert_is_dynamic(tfg, smb, dyn, seeds, fanouts):
    """smb (static, over `seeds` with dead slots) against dyn (sample_blocks of the live seeds, same seed): test 1's mapping."""
    L = len(dyn.blocks)
    ks = [int(k) for k in fanouts[len(fanouts) - L:]]
    cap = tfg.utils.static_capacities(len(seeds), ks) if ks else None
    live = smb.live
    assert live.dtype == torch.bool and torch.equal(live, smb.node_index >= 0)
    assert torch.equal(smb.node_index[live], dyn.node_index)
    assert torch.equal(smb.seed_mask, live[:len(seeds)]) and smb.seed_mask.cpu().tolist() == [s >= 0 for s in seeds]
    assert smb.num_host_syncs == 0 and smb.num_seeds == len(seeds) and len(smb.blocks) == L
    rank = _rank(live)
    counts = smb.counts.cpu().numpy()
    assert counts.shape == (L, 2)
    if cap is not None:
        assert smb.node_index.shape[0] == cap.rows[-1] and smb.capacities == cap
    for l, (b, d) in enumerate(zip(smb.blocks, dyn.blocks)):
        h = L - 1 - l                                          # the hop's index, 0 = next to the seeds
        R, E, Rn, k = cap.rows[h], cap.edges[h], cap.rows[h + 1], cap.fanouts[h]
        assert (b.num_dst, b.num_src) == (R, Rn) and tuple(b.edge_index.shape) == (2, E) and tuple(b.edge_weight.shape) == (E,)
        assert b.edge_index.dtype == torch.int32 and b.edge_weight.dtype == torch.float32
        total, n_new = int(counts[h, 0]), int(counts[h, 1])
        assert total == d.num_edges and n_new == d.num_src - d.num_dst
        assert torch.equal(rank[b.edge_index[:, :total].long()], d.edge_index)
        assert torch.equal(b.edge_weight[:total], d.edge_weight)                  # bit for bit
        # the tail: unit self-loops on the sink rows R + E, R + E + 1, ..., k per sink
        t = torch.arange(E - total, device=live.device)
        sink = (R + E + t // max(k, 1)).to(torch.int32)
        assert torch.equal(b.edge_index[0, total:], sink) and torch.equal(b.edge_index[1, total:], sink)
        assert bool((b.edge_weight[total:] == 1.0).all())
        assert not bool(live[R + n_new:Rn].any()) and bool(live[R:R + n_new].all())
    for inner, outer in zip(smb.blocks[1:], smb.blocks[:-1]):
        assert inner.num_src == outer.num_dst
    if L:
        assert smb.blocks[-1].num_dst == len(seeds) and smb.blocks[0].num_src == smb.node_index.numel()


def _assert_is_mirror(smb, want):
    assert np.array_equal(smb.node_index.cpu().numpy(), want["node_index"])
    assert np.array_equal(smb.counts.cpu().numpy(), want["counts"])
    for b, w in zip(smb.blocks, want["blocks"]):
        assert (b.num_dst, b.num_src) == (w["num_dst"], w["num_src"])
        assert np.array_equal(b.edge_index.cpu().numpy(), w["edge_index"])
        assert np.array_equal(b.edge_weight.cpu().numpy(), w["edge_weight"])


# ---- 1. it is sample_blocks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fanouts, padding", CASES, ids=lambda v: str(v))
def test_static_blocks_are_sample_blocks_of_the_live_seeds(tfg, world, fanouts, padding):
    s = world["sampler"]
    smb = s.sample_blocks_static(SEEDS, fanouts, padding=padding, seed=77)
    dyn = s.sample_blocks(LIVE, fanouts, padding=padding, seed=77)
    _assert_is_dynamic(tfg, smb, dyn, SEEDS, fanouts)
    _assert_is_mirror(smb, mirror_static_blocks(_mirror_of(world, dyn, LIVE, fanouts, padding), SEEDS, fanouts))
    smb.check()                                                  # nothing to report
    # the seeds as a device tensor, the seed as a device word: the same minibatch; another seed: another one
    again = s.sample_blocks_static(torch.tensor(SEEDS, device=world["dev"]), fanouts, padding=padding,
                                   seed=torch.full((1,), 77, dtype=torch.int64, device=world["dev"]))
    assert torch.equal(again.node_index, smb.node_index)
    for a, b in zip(again.blocks, smb.blocks):
        assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.edge_weight, b.edge_weight)
    other = s.sample_blocks_static(SEEDS, fanouts, padding=padding, seed=78)
    assert not torch.equal(other.node_index, smb.node_index) or any(
        not torch.equal(a.edge_index, b.edge_index) for a, b in zip(other.blocks, smb.blocks))
    # no row of a block is longer than its fan-out
    from tf_geometric_amd.plan import attached_plan
    for l, b in enumerate(smb.blocks):
        if b.num_edges:
            assert int(attached_plan(b.edge_index).in_degree().max()) <= fanouts[l]


def test_the_fused_static_minibatch_is_the_fused_dynamic_one(tfg, world):
    s = world["sampler"]
    for fanouts, padding in (([5], False), ([5, 3], True), ([40, 5, 2], False)):
        smb = s.sample_blocks_static(SEEDS, fanouts, padding=padding, seed=77, fuse_input_hop=True)
        dyn = s.sample_blocks(LIVE, fanouts, padding=padding, seed=77, fuse_input_hop=True)
        assert smb.input_hop == (fanouts[0], padding, len(fanouts) - 1) and len(smb.blocks) == len(fanouts) - 1
        _assert_is_dynamic(tfg, smb, dyn, SEEDS, fanouts)
        unfused = s.sample_blocks_static(SEEDS, fanouts, padding=padding, seed=77)
        assert torch.equal(smb.node_index, unfused.node_index[:smb.node_index.numel()])
        for a, b in zip(smb.blocks, unfused.blocks[1:]):
            assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.edge_weight, b.edge_weight)


# ---- 2. the plans -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fanouts, padding", [([5, 3], False), ([40, 5, 2], True), ([3, 0], False)], ids=lambda v: str(v))
def test_both_attached_plans_equal_the_built_ones(tfg, world, fanouts, padding):
    from tf_geometric_amd.plan import CsrPlan, attached_plan
    smb = world["sampler"].sample_blocks_static(SEEDS, fanouts, padding=padding, seed=5)
    for l, b in enumerate(smb.blocks):
        n = b.num_src
        plan = attached_plan(b.edge_index)
        assert plan is not None and (plan.n_dst, plan.n_src, plan.num_edges) == (n, n, b.num_edges)
        assert plan.padded_to(n, n) is plan                      # what a layer called on h[:num_src] asks for
        built = CsrPlan.build(b.edge_index, n, n)
        for name in ("row_ptr", "col", "perm"):
            assert torch.equal(getattr(plan, name), getattr(built, name)), (l, name)
        pt = plan._transposed
        assert pt is not None and pt._transposed is plan and plan.transposed() is pt
        built_t = CsrPlan.build(torch.stack([b.edge_index[1], b.edge_index[0]]), n, n)
        assert (pt.n_dst, pt.n_src, pt.num_edges) == (n, n, b.num_edges)
        for name in ("row_ptr", "col", "perm"):
            assert torch.equal(getattr(pt, name), getattr(built_t, name)), (l, "transposed " + name)
        # no destination row is longer than the fan-out: no hub rows, no walk order, neither computed
        assert plan._hub is False and plan._row_order is False and plan.hub_info() is None and plan.row_order() is None


def _static_model(tfg, kind, weights, world_m, seeds, fanouts, fused, g_rows, count_builds=None):
    """Two layers over a static minibatch of `seeds`; loss = sum(out * g * seed_mask).  (seed-row outputs, gradients, mb)."""
    ei, ew, x, _, _ = world_m
    dev = tfg._lib.device()
    sampler = tfg.utils.RandomNeighborSampler(torch.from_numpy(ei).to(dev), torch.from_numpy(ew).to(dev))
    if count_builds is not None:
        count_builds["n"] = 0                                    # the sampler's own plan of the whole graph is not the point
    mb = sampler.sample_blocks_static(seeds, fanouts, seed=9, fuse_input_hop=fused)
    layers = _layers(tfg, kind, weights)
    for layer, w in zip(layers, weights):
        layer._maybe_build([torch.empty(1, next(iter(w.values())).shape[0])])
        layer.set_weights(**w)
    x_t = torch.from_numpy(x).to(dev)
    h = mb.gather(x_t)
    rest = layers
    if fused:
        h = layers[0].combine([h, mb.input_aggregate(x_t, kind)], training=True)
        rest = layers[1:]
    for layer, b in zip(rest, mb.blocks):
        h = layer([h[:b.num_src], b.edge_index, b.edge_weight], training=True)[:b.num_dst]
    out = h[:mb.num_seeds]
    g_t = torch.from_numpy(g_rows[:, :out.shape[1]]).to(dev)
    (out * g_t * mb.seed_mask[:, None]).sum().backward()
    torch.cuda.synchronize()
    grads = [{k: getattr(layer, k).grad.cpu().numpy() for k in w} for layer, w in zip(layers, weights)]
    return out.detach()[mb.seed_mask].cpu().numpy(), grads, mb


def test_forward_and_backward_build_no_plan(tfg, monkeypatch):
    from tf_geometric_amd import plan as P
    count = {"n": 0}
    real = P.CsrPlan.build

    def counted(*a, **kw):
        count["n"] += 1
        return real(*a, **kw)

    world_m = _model_world(tfg)
    weights = _weights("mean", np.random.Generator(np.random.PCG64(31)))
    seeds, g = world_m[3], world_m[4]
    monkeypatch.setattr(P.CsrPlan, "build", staticmethod(counted))
    _static_model(tfg, "mean", weights, world_m, seeds, [5, 3], False, g, count_builds=count)
    assert count["n"] == 0, "forward and backward built {} plans".format(count["n"])


# ---- 3. no host reads ---------------------------------------------------------------------------------------------------
def _sync_warnings(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]


@pytest.mark.parametrize("kind", ["mean", "sum"])
@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_sampling_gather_and_a_forward_read_nothing_back(tfg, world, kind, fused):
    s, dev = world["sampler"], world["dev"]
    seeds = torch.tensor(SEEDS, dtype=torch.int32, device=dev)
    state = torch.full((1,), 3, dtype=torch.int64, device=dev)
    x = torch.randn(401, 12, device=dev)
    cls = tfg.layers.MeanGraphSage if kind == "mean" else tfg.layers.SumGraphSage
    layers = [cls(16, activation=tfg.relu, concat=True), cls(8, activation=None, concat=True)]

    def run():
        mb = s.sample_blocks_static(seeds, [5, 3], seed=state, fuse_input_hop=fused)
        h = mb.gather(x)
        rest = layers
        if fused:
            h = layers[0].combine([h, mb.input_aggregate(x, kind)])
            rest = layers[1:]
        for layer, b in zip(rest, mb.blocks):
            h = layer([h[:b.num_src], b.edge_index, b.edge_weight])[:b.num_dst]
        return mb, h

    run()                                                        # warm: weights, allocator, first launches
    (mb, h), reads = _sync_warnings(run)
    assert reads == [] and mb.num_host_syncs == 0, reads
    assert tuple(h.shape) == (len(SEEDS), 8)
    _, reads = _sync_warnings(mb.check)
    assert len(reads) == 1, reads


# ---- 4. gather and input_aggregate --------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 4, 100, "strided"])
def test_gather_and_input_aggregate_rows(tfg, world, F):
    s, dev = world["sampler"], world["dev"]
    gen = torch.Generator().manual_seed(4)
    if F == "strided":                                           # a column block of a wider table: ldx = 103, not a multiple of 4
        x = torch.randn(401, 103, generator=gen).to(dev)[:, :100]
        assert x.stride(0) % 4 != 0
    else:
        x = torch.randn(401, F, generator=gen).to(dev)
    for fanouts, padding in (([5, 3], False), ([40, 3], True)):
        smb = s.sample_blocks_static(SEEDS, fanouts, padding=padding, seed=21, fuse_input_hop=True)
        dyn = s.sample_blocks(LIVE, fanouts, padding=padding, seed=21, fuse_input_hop=True)
        live = smb.live
        assert not bool(live.all()) and bool(live.any())
        got = smb.gather(x)
        assert got.dtype == torch.float32 and tuple(got.shape) == (smb.node_index.numel(), x.shape[1])
        assert torch.equal(got[live], x[smb.node_index[live].long()]) and torch.equal(got[live], dyn.gather(x))
        assert int((got[~live] != 0).sum()) == 0                 # exact zeros, +0.0
        assert not bool(torch.signbit(got[~live]).any())
        for op in ("mean", "sum"):
            agg = smb.input_aggregate(x, op)
            assert tuple(agg.shape) == tuple(got.shape)
            assert torch.equal(agg[live], dyn.input_aggregate(x, op))             # bit for bit
            assert int((agg[~live] != 0).sum()) == 0
        smb.check()                                              # dead rows raised no flag
    # a table that is being trained goes through torch's indexing and carries the gradient; dead rows give and take nothing
    xg = x.clone().contiguous().requires_grad_(True)
    got = smb.gather(xg)
    assert torch.equal(got.detach(), smb.gather(x))
    got.sum().backward()
    want = torch.zeros(401, device=dev).index_add_(0, smb.node_index[live].long(), torch.ones(int(live.sum()), device=dev))
    assert torch.equal(xg.grad[:, 0], want)
    with pytest.raises(ValueError, match="composed dynamic route"):
        smb.input_aggregate(xg, "mean")
    with pytest.raises(ValueError, match="fuse_input_hop=True"):
        s.sample_blocks_static(SEEDS, [5, 3], seed=21).input_aggregate(x)


# ---- 5. models ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("kind", ["mean", "sum"])
def test_two_layers_on_the_static_blocks_equal_the_full_graph_in_float64(tfg, kind, fused):
    world_m = _model_world(tfg)
    weights = _weights(kind, np.random.Generator(np.random.PCG64(31)))
    ei, ew, x, seeds, g = world_m
    ref_out, ref_grads = _f64_model(kind, x, ei, ew, weights, seeds, g)
    # dead slots in front, in the middle and at the end; their rows of g are NOT zero: the mask has to remove them
    slots = [-1] + list(seeds[:10]) + [-1, -1] + list(seeds[10:]) + [-1]
    live_at = [i for i, v in enumerate(slots) if v >= 0]
    g_slots = np.full((len(slots), g.shape[1]), 3.0, dtype=np.float32)
    g_slots[live_at] = g
    fanouts = [150, 150]                                         # at the largest degree: every neighbour is kept
    out, grads, mb = _static_model(tfg, kind, weights, world_m, np.asarray(slots), fanouts, fused, g_slots)
    assert int(mb.seed_mask.sum()) == 32 and mb.num_seeds == len(slots) == 36
    _close(out, ref_out, "{} static out".format(kind))
    for i, (got, ref) in enumerate(zip(grads, ref_grads)):
        assert sorted(got) == sorted(ref)
        for k in sorted(ref):
            _close(got[k], ref[k], "{} static layer {} d/d{}".format(kind, i, k))
    # dead seeds contribute nothing: the live-only batch gives the same gradients
    out_l, grads_l, mb_l = _static_model(tfg, kind, weights, world_m, np.asarray(seeds), fanouts, fused, g)
    assert bool(mb_l.seed_mask.all())
    _close(out, out_l, "{} out with dead slots vs live only".format(kind))
    for i, (got, ref) in enumerate(zip(grads, grads_l)):
        for k in sorted(ref):
            _close(got[k], ref[k], "{} layer {} d/d{} with dead slots vs live only".format(kind, i, k))


# ---- 6. clean table, flags ----------------------------------------------------------------------------------------------
def test_the_table_is_clean_and_bad_seeds_are_dead_slots(tfg, world):
    L = tfg._lib
    s = tfg.utils.RandomNeighborSampler(world["ei"], world["ew"])
    good = s.sample_blocks_static(SEEDS, [5, 3], seed=1)
    assert int((s._nbrblock.table != L.NBRBLOCK_EMPTY).sum()) == 0
    good.check()
    cases = (([HUB, 17, 3, 17, 7], 3, "repeat", [HUB, 17, 3, 7]),                       # the FIRST occurrence stays live
             ([HUB, 401, 3], 1, r"outside \[0, 401\)", [HUB, 3]),
             ([HUB, -2, 3], 1, r"outside \[0, 401\)", [HUB, 3]),
             (np.asarray([3, 2 ** 33 + 4, 9]), 1, r"outside \[0, 401\)", [3, 9]))
    for seeds, dead_at, word, live_seeds in cases:
        mb = s.sample_blocks_static(seeds, [5, 3], seed=1)         # does not raise
        assert int((s._nbrblock.table != L.NBRBLOCK_EMPTY).sum()) == 0, seeds
        with pytest.raises(ValueError, match=word):
            mb.check()
        assert not bool(mb.seed_mask[dead_at]) and int(mb.node_index[dead_at]) == -1
        assert int(mb.seed_mask.sum()) == len(live_seeds)
        # the rest of the minibatch is the one of the good seeds
        assert torch.equal(mb.node_index[mb.live], s.sample_blocks(live_seeds, [5, 3], seed=1).node_index)
        # and the next good call is a fresh sampler's
        again = s.sample_blocks_static(SEEDS, [5, 3], seed=1)
        assert torch.equal(again.node_index, good.node_index)
        assert all(torch.equal(a.edge_index, b.edge_index) for a, b in zip(again.blocks, good.blocks))
    # a device seed of the wrong kind is refused before any launch
    with pytest.raises(ValueError, match="one int64"):
        s.sample_blocks_static(SEEDS, [5], seed=torch.zeros(1, dtype=torch.int32, device=world["dev"]))


# ---- 7. capture ---------------------------------------------------------------------------------------------------------
def test_a_captured_sampler_draws_a_fresh_sample_per_replay(tfg, world):
    """7(a): the seed is a device word the captured sequence advances; the seeds are a buffer rewritten between replays."""
    dev = world["dev"]
    s = tfg.utils.RandomNeighborSampler(world["ei"], world["ew"])
    fanouts = [5, 3]
    lists = [SEEDS, [7, -1, 399, 5, HUB, 123, -1, -1], [SINK, 1, 2, 3, 4, 5, 6, ISOLATED]]
    seeds_buf = torch.tensor(lists[0], dtype=torch.int32, device=dev)
    state = torch.full((1,), 100, dtype=torch.int64, device=dev)
    s.sample_blocks_static(seeds_buf, fanouts, seed=state)       # the sampler's state exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        smb = s.sample_blocks_static(seeds_buf, fanouts, seed=state)
        state.add_(1)
    kept = []
    for r, seeds in enumerate(lists):
        seeds_buf.copy_(torch.tensor(seeds, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert int(state) == 101 + r
        dyn = s.sample_blocks([v for v in seeds if v >= 0], fanouts, seed=100 + r)
        _assert_is_dynamic(tfg, smb, dyn, seeds, fanouts)
        smb.check()
        assert int((s._nbrblock.table != tfg._lib.NBRBLOCK_EMPTY).sum()) == 0
        kept.append([b.edge_index.clone() for b in smb.blocks])
    assert any(not torch.equal(a, b) for a, b in zip(kept[0], kept[1]))
    # the same seeds again at the next seed value: another sample
    seeds_buf.copy_(torch.tensor(lists[2], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    assert any(not torch.equal(a, b.edge_index) for a, b in zip(kept[2], smb.blocks))


def test_a_captured_training_step_that_samples_equals_the_eager_steps(tfg):
    """7(b): CapturedTrainStep over a loss_fn that samples; three replays against three eager static steps, same seeds."""
    world_m = _model_world(tfg)
    ei, ew, x, seeds, g = world_m
    dev = tfg._lib.device()
    weights = _weights("mean", np.random.Generator(np.random.PCG64(31)))
    slots = torch.tensor(list(seeds[:20]) + [-1, -1] + list(seeds[20:]), dtype=torch.int32, device=dev)
    g_t = torch.from_numpy(np.concatenate([g[:20, :8], np.ones((2, 8), np.float32), g[20:, :8]])).to(dev)
    x_t = torch.from_numpy(x).to(dev)
    sampler = tfg.utils.RandomNeighborSampler(torch.from_numpy(ei).to(dev), torch.from_numpy(ew).to(dev))
    state = torch.full((1,), 500, dtype=torch.int64, device=dev)

    def make():
        layers = _layers(tfg, "mean", weights)
        for layer, w in zip(layers, weights):
            layer._maybe_build([torch.empty(1, next(iter(w.values())).shape[0])])
            layer.set_weights(**w)
        opt = torch.optim.Adam([p for layer in layers for p in layer.parameters()], lr=1e-2, capturable=True)
        return layers, opt

    def loss_of(layers):
        mb = sampler.sample_blocks_static(slots, [5, 3], seed=state)
        state.add_(1)
        h = mb.gather(x_t)
        for layer, b in zip(layers, mb.blocks):
            h = layer([h[:b.num_src], b.edge_index, b.edge_weight], training=True)[:b.num_dst]
        return (h[:mb.num_seeds] * g_t * mb.seed_mask[:, None]).sum()

    layers, opt = make()
    eager = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss = loss_of(layers)
        loss.backward()
        opt.step()
        eager.append(float(loss.detach()))
    assert int(state) == 503 and len(set(eager)) == 3
    layers, opt = make()
    step = tfg.CapturedTrainStep(lambda: loss_of(layers), opt)
    state.fill_(500)                                             # the warm-up steps advanced the seed: start where eager did
    captured = [float(step().detach()) for _ in range(3)]
    assert int(state) == 503
    print("eager    ", eager)
    print("captured ", captured, " bit-equal:", captured == eager)
    _close(captured, eager, "captured vs eager losses")


def test_seed_none_and_a_first_call_are_refused_inside_a_capture(tfg, world, monkeypatch):
    """7(c), with the capture state faked as tests/test_gpu_nbrblock.py does: both refusals come before any launch."""
    s = tfg.utils.RandomNeighborSampler(world["ei"], world["ew"])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="call it once eagerly before the capture"):
        s.sample_blocks_static(SEEDS, [5], seed=1)
    monkeypatch.undo()
    s.sample_blocks_static(SEEDS, [5], seed=1)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="seed=None inside a hipGraph capture"):
        s.sample_blocks_static(SEEDS, [5])
    assert int((s._nbrblock.table != tfg._lib.NBRBLOCK_EMPTY).sum()) == 0


def test_the_demo_trains_from_a_captured_step():
    """examples/demo_graph_sage_minibatch.py --capture: three short epochs replayed from one hipGraph, the short last batch of
    an epoch as dead slots under the masked loss."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("demo_graph_sage_minibatch_static",
                                                  os.path.join(ROOT, "examples", "demo_graph_sage_minibatch.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    acc, loss = demo.main(epochs=3, batch=512, num_nodes=4000, quiet=True, fuse_input_hop=True, capture=True)
    print("captured demo: test accuracy {:.3f}, last loss {:.3f}".format(acc, loss))
    assert np.isfinite(loss) and acc > 1.0 / 6        # six planted classes: better than chance after three short epochs
