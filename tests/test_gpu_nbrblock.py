# coding=utf-8
"""Minibatch neighbour sampling on the GPU (include/tfgx_nbrblock.h, RandomNeighborSampler.sample_rows / sample_blocks).

One graph serves the sampling tests: 401 nodes and about 12 k edges, built so that every branch of the per-row sampler is taken
— in-degrees 0, 1, 4 / 5 / 6 (around k = 5), 20 and 33 (Floyd at k = 5, the keep / selection boundary at k = 32, 33), 100
(selection sampling at k = 40) and one hub of 5000 (the wave-per-row path at k = 40 and ratio = 0.5) — with a sink node whose id
is larger than every row id, random weights, self-loops and duplicate edges.

  1. sample_rows is exactly the slices of the whole-graph sample() — the expected value comes from the existing entry point.
  2. sample_blocks is exactly mirror_blocks (tests/test_nbrblock_abi.py) fed the whole-graph sample() of every hop.
  3. The relabel table is clean after every call, refused calls included.
  4. Two layers over the blocks with fan-outs that keep every neighbour equal the same layers computed full-graph in float64.
  5. The attached plans are used: the forward pass builds no plan, the backward at most the transposed one per block.
"""
import numpy as np
import pytest
import torch

from test_nbrblock_abi import mirror_blocks, lists_of

pytestmark = pytest.mark.gpu

HUB, ISOLATED, SINK = 8, 0, 400
DEGREES = {0: 0, 1: 1, 2: 4, 3: 5, 4: 6, 5: 20, 6: 33, 7: 100, 8: 5000}


def _graph():
    rng = np.random.Generator(np.random.PCG64(11))
    n_rows = 400                                   # rows 0 .. 399; node 400 only ever appears as a neighbour
    rows, cols = [], []
    for r in range(n_rows):
        d = DEGREES.get(r, int(rng.integers(8, 28)))
        c = rng.integers(0, n_rows, d)             # with repeats: duplicate edges happen (the hub has thousands)
        rows.append(np.full(d, r))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    for r in (3, 6, 7, 8, 50, 51):                 # self-loops
        cols[np.nonzero(rows == r)[0][0]] = r
    for r in (2, 5, 8, 60, 399):                   # the sink as a neighbour, of the hub and of the last row among others
        cols[np.nonzero(rows == r)[0][-1]] = SINK
    order = rng.permutation(rows.shape[0])         # the caller's edge order is not sorted
    ei = np.stack([rows[order], cols[order]]).astype(np.int32)
    ew = rng.uniform(0.25, 2.0, ei.shape[1]).astype(np.float32)
    return ei, ew


@pytest.fixture(scope="module")
def world(tfg):
    ei, ew = _graph()
    dev = tfg._lib.device()
    ei_t, ew_t = torch.from_numpy(ei).to(dev), torch.from_numpy(ew).to(dev)
    sampler = tfg.utils.RandomNeighborSampler(ei_t, ew_t)
    deg = np.bincount(ei[0], minlength=401)
    assert all(deg[r] == d for r, d in DEGREES.items()) and deg[SINK] == 0 and ei[1].max() == SINK and ei[0].max() == 399
    assert 11000 < ei.shape[1] < 13500
    return {"ei": ei_t, "ew": ew_t, "sampler": sampler, "full": {}}


def _full(world, seed, **kw):
    """The whole-graph sample of the EXISTING entry point, split by row (computed once per argument set, never changed)."""
    key = (seed,) + tuple(sorted(kw.items()))
    if key not in world["full"]:
        ei, ew = world["sampler"].sample(seed=seed, **kw)
        world["full"][key] = lists_of(None if ei is None else ei.cpu().numpy(), None if ew is None else ew.cpu().numpy())
    return world["full"][key]


def _expected_rows(lists, rows):
    pos, col, w = [], [], []
    for i, r in enumerate(rows):
        c, ww = lists.get(int(r), (np.zeros(0, np.int32), np.zeros(0, np.float32)))
        pos.append(np.full(len(c), i, np.int32))
        col.append(np.asarray(c, np.int32))
        w.append(np.asarray(ww, np.float32))
    cat = lambda parts, dt: np.concatenate(parts + [np.zeros(0, dt)]).astype(dt)        # noqa: E731
    return np.stack([cat(pos, np.int32), cat(col, np.int32)]), cat(w, np.float32)


def _row_lists():
    rng = np.random.Generator(np.random.PCG64(5))
    subset = rng.permutation(401)[:150]
    if HUB not in subset:
        subset[0] = HUB
    return {"all": np.arange(401), "shuffled subset": subset, "repeated id": np.asarray([7, HUB, 3, 7, SINK, HUB, 6, 7]),
            "isolated and sink": np.asarray([SINK, ISOLATED, SINK, ISOLATED]), "empty": np.zeros(0, np.int64)}


# ---- 1. sample_rows against the full-graph sampler ----------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 2 ** 61 + 12345])
@pytest.mark.parametrize("kw", [dict(k=5), dict(k=32), dict(k=33), dict(k=40), dict(ratio=0.5), dict(k=8, padding=True)],
                         ids=lambda kw: "-".join("{}={}".format(*i) for i in kw.items()))
def test_sample_rows_is_the_slice_of_the_full_graph_sample(world, kw, seed):
    s = world["sampler"]
    lists = _full(world, seed, **kw)
    for name, rows in _row_lists().items():
        want_ei, want_w = _expected_rows(lists, rows)
        ei, ew = s.sample_rows(rows, seed=seed, **kw)
        assert ei.dtype == torch.int32 and ew.dtype == torch.float32 and tuple(ei.shape) == (2, want_ei.shape[1]), name
        assert np.array_equal(ei.cpu().numpy(), want_ei), (name, kw)
        assert np.array_equal(ew.cpu().numpy(), want_w), (name, kw)            # bit for bit: the same float32 weights
        ei2, ew2 = s.sample_rows(torch.as_tensor(rows).to(ei.device), seed=seed, **kw)
        assert torch.equal(ei, ei2) and torch.equal(ew, ew2), name
        if rows.size:
            assert bool((ei[0][1:] >= ei[0][:-1]).all())
    # the branches the graph was built for were taken: the hub's row is long, and it is not kept whole
    if kw.get("k") == 40:
        assert len(lists[HUB][0]) == 40 and len(lists[7][0]) == 40 and len(lists[6][0]) == 33
    if "ratio" in kw:
        assert len(lists[HUB][0]) == 2500 and len(lists[7][0]) == 50
    if kw.get("padding"):
        assert len(lists[1][0]) == 8 and len(set(lists[1][0].tolist())) == 1 and ISOLATED not in lists


def test_sample_rows_refuses_ids_outside_the_graph(world):
    s = world["sampler"]
    for rows in ([1, 401], [-1, 2], np.asarray([5, 2 ** 40]), torch.tensor([3, 401], dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"outside \[0, 401\)"):
            s.sample_rows(rows, k=5, seed=1)
    ei, ew = s.sample_rows([SINK, ISOLATED], k=5, seed=1)           # valid nodes without neighbours: [2, 0], not None
    assert tuple(ei.shape) == (2, 0) and tuple(ew.shape) == (0,)


def test_sampling_is_refused_inside_a_capture(world, monkeypatch):
    """The sizes of a sample are read back to the host: both calls refuse a capturing stream before they launch anything."""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="hipGraph capture"):
        world["sampler"].sample_rows([1, 2], k=5, seed=1)
    with pytest.raises(RuntimeError, match="hipGraph capture"):
        world["sampler"].sample_blocks([1, 2], [5], seed=1)


# ---- 2. sample_blocks against the mirror --------------------------------------------------------------------------------
SEEDS = [HUB, 17, ISOLATED, SINK, 7, 399, 5, 123]


def _mirror_of(world, mb, seeds, fanouts, padding=False):
    hops = []
    for h in range(len(fanouts)):
        kw = dict(k=fanouts[len(fanouts) - 1 - h])
        if padding:
            kw["padding"] = True
        hops.append(_full(world, mb.hop_seeds[h], **kw))
    return mirror_blocks(seeds, hops)


def _assert_is_mirror(tfg, mb, m, seeds):
    from tf_geometric_amd.plan import CsrPlan, attached_plan
    node_index = mb.node_index.cpu().numpy()
    assert mb.node_index.dtype == torch.int32 and np.array_equal(node_index, m["node_index"])
    assert mb.num_seeds == len(seeds) and list(node_index[:len(seeds)]) == list(seeds)
    assert len(set(node_index.tolist())) == len(node_index)
    assert len(mb.blocks) == len(m["blocks"])
    for b, want in zip(mb.blocks, m["blocks"]):
        assert (b.num_dst, b.num_src) == (want["num_dst"], want["num_src"])
        assert b.edge_index.dtype == torch.int32 and np.array_equal(b.edge_index.cpu().numpy(), want["edge_index"])
        assert np.array_equal(b.edge_weight.cpu().numpy(), want["edge_weight"])
        plan = attached_plan(b.edge_index)
        assert plan is not None and (plan.n_dst, plan.n_src, plan.num_edges) == (b.num_dst, b.num_src, b.num_edges)
        assert np.array_equal(plan.row_ptr.cpu().numpy(), want["row_ptr"]) and np.array_equal(plan.col.cpu().numpy(), want["col"])
        built = CsrPlan.build(b.edge_index, b.num_dst, b.num_src)
        assert torch.equal(built.row_ptr, plan.row_ptr) and torch.equal(built.col, plan.col)
        assert torch.equal(built.perm, plan.perm)                 # already grouped by destination: the stable sort moves nothing
    assert mb.blocks[-1].num_dst == len(seeds) and mb.blocks[0].num_src == len(node_index)
    for inner, outer in zip(mb.blocks[1:], mb.blocks[:-1]):
        assert inner.num_src == outer.num_dst


@pytest.mark.parametrize("fanouts, padding", [([5], False), ([5, 3], False), ([40, 5, 2], False), ([5, 3], True)])
def test_sample_blocks_is_the_mirror(tfg, world, fanouts, padding):
    s = world["sampler"]
    mb = s.sample_blocks(SEEDS, fanouts, padding=padding, seed=77)
    assert mb.hop_seeds == [tfg.utils.hop_seed(77, h) for h in range(len(fanouts))]
    assert mb.num_host_syncs == len(fanouts) + 1
    _assert_is_mirror(tfg, mb, _mirror_of(world, mb, SEEDS, fanouts, padding), SEEDS)
    # a second sampler object gives the same minibatch; another seed does not
    other = tfg.utils.RandomNeighborSampler(world["ei"], world["ew"]).sample_blocks(torch.tensor(SEEDS), fanouts,
                                                                                     padding=padding, seed=77)
    assert torch.equal(other.node_index, mb.node_index)
    for a, b in zip(other.blocks, mb.blocks):
        assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.edge_weight, b.edge_weight)
    diff = s.sample_blocks(SEEDS, fanouts, padding=padding, seed=78)
    assert any(a.edge_index.shape != b.edge_index.shape or not torch.equal(a.edge_index, b.edge_index)
               for a, b in zip(diff.blocks, mb.blocks))
    _assert_is_mirror(tfg, diff, _mirror_of(world, diff, SEEDS, fanouts, padding), SEEDS)


def test_sample_blocks_with_a_zero_fanout_and_without_seeds(tfg, world):
    s = world["sampler"]
    mb = s.sample_blocks(SEEDS, [3, 0], seed=5)                    # the hop next to the seeds is empty
    _assert_is_mirror(tfg, mb, _mirror_of(world, mb, SEEDS, [3, 0]), SEEDS)
    assert mb.blocks[1].num_edges == 0 and mb.blocks[1].num_src == len(SEEDS) and mb.blocks[0].num_edges > 0
    none = s.sample_blocks([], [5, 3], seed=5)
    assert none.node_index.numel() == 0 and [b.num_edges for b in none.blocks] == [0, 0] and none.num_seeds == 0
    x = torch.arange(401 * 3, dtype=torch.float32, device=mb.node_index.device).reshape(401, 3)
    assert torch.equal(mb.gather(x), x[mb.node_index.long()])


def test_sample_blocks_reads_back_once_per_hop_plus_once(world):
    """torch's synchronisation debug mode reports every synchronising call: with the seeds already on the device a call over L
    hops makes L + 1 of them — the reads it counts itself — and nothing hidden (no torch.unique, no nonzero, no sized
    repeat_interleave)."""
    import warnings
    s = world["sampler"]
    seeds = torch.tensor(SEEDS, dtype=torch.int32, device=world["ei"].device)
    for fanouts in ([5], [5, 3], [40, 5, 2]):
        s.sample_blocks(seeds, fanouts, seed=3)                  # warm: allocator, first launches
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                mb = s.sample_blocks(seeds, fanouts, seed=3)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        reads = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
        assert len(reads) == len(fanouts) + 1 == mb.num_host_syncs, reads


# ---- 3. the table is clean after every call -----------------------------------------------------------------------------
def _same(a, b):
    return torch.equal(a.node_index, b.node_index) and all(
        torch.equal(p.edge_index, q.edge_index) and torch.equal(p.edge_weight, q.edge_weight) and
        (p.num_dst, p.num_src) == (q.num_dst, q.num_src) for p, q in zip(a.blocks, b.blocks))


def test_the_table_is_clean_after_every_call(tfg, world):
    fresh = lambda: tfg.utils.RandomNeighborSampler(world["ei"], world["ew"])        # noqa: E731
    A, B = ([HUB, 3, SINK, 250], [5, 3]), ([250, 9, 3, 77, 6], [40, 2])
    want_a, want_b = fresh().sample_blocks(*A, seed=1), fresh().sample_blocks(*B, seed=2)
    s = fresh()
    assert _same(s.sample_blocks(*A, seed=1), want_a) and _same(s.sample_blocks(*B, seed=2), want_b)
    assert _same(s.sample_blocks(*A, seed=1), want_a)
    s = fresh()
    assert _same(s.sample_blocks(*B, seed=2), want_b) and _same(s.sample_blocks(*A, seed=1), want_a)
    assert int((s._nbrblock.table != tfg._lib.NBRBLOCK_EMPTY).sum()) == 0
    # refused calls: a duplicate seed, a seed >= n_nodes, a negative seed — each found on the device, each a ValueError, and
    # the next good call equals a fresh sampler's
    for bad, word in (([3, HUB, 9, 3], "repeat"), ([3, 401, 9], r"outside \[0, 401\)"), ([3, -1, 9], r"outside \[0, 401\)"),
                      (np.asarray([3, 2 ** 33 + 4]), r"outside \[0, 401\)")):
        with pytest.raises(ValueError, match=word):
            s.sample_blocks(bad, [5, 3], seed=1)
        assert _same(s.sample_blocks(*A, seed=1), want_a), bad
        assert int((s._nbrblock.table != tfg._lib.NBRBLOCK_EMPTY).sum()) == 0


# ---- 4. a model on the blocks -------------------------------------------------------------------------------------------
N_M, F_M, BIG_ROW = 200, 12, 40


def _model_world(tfg):
    rng = np.random.Generator(np.random.PCG64(21))
    deg = rng.integers(2, 11, N_M)                 # mean degree 6
    deg[BIG_ROW] = 150
    rows = np.repeat(np.arange(N_M), deg)
    cols = rng.integers(0, N_M, rows.shape[0])
    order = rng.permutation(rows.shape[0])
    ei = np.stack([rows[order], cols[order]]).astype(np.int32)
    ew = rng.uniform(0.5, 1.5, ei.shape[1]).astype(np.float32)
    x = rng.standard_normal((N_M, F_M)).astype(np.float32)
    seeds = rng.permutation(N_M)[:32]
    if BIG_ROW not in seeds:
        seeds[3] = BIG_ROW
    g = rng.standard_normal((32, 64)).astype(np.float32)
    return ei, ew, x, seeds, g


def _f64_aggregate(kind, h, row, col, w, n):
    """Full-graph float64 aggregation of a layer, written out: mean / sum of w_e * h[col_e] over the in-edges of row_e
    (nn/conv/graph_sage.py:9-115), or D^-1 (A + I) h (nn/conv/gcn.py:71-72, :101-109 with norm='left')."""
    s = torch.zeros(n, h.shape[1], dtype=torch.float64).index_add(0, row, w[:, None] * h[col])
    if kind == "sum":
        return s
    if kind == "mean":
        cnt = torch.bincount(row, minlength=n).clamp(min=1).double()
        return s / cnt[:, None]
    deg = torch.zeros(n, dtype=torch.float64).index_add(0, row, w) + 1.0
    return (s + h) / deg[:, None]


def _f64_model(kind, x, ei, ew, weights, seeds, g):
    """Both layers over the WHOLE graph in float64 on the CPU, read at the seed rows; gradients of sum(out[seeds] * g)."""
    row, col = torch.from_numpy(ei[0]).long(), torch.from_numpy(ei[1]).long()
    w = torch.from_numpy(ew).double()
    leaves = [{k: torch.from_numpy(v).double().requires_grad_(True) for k, v in layer.items()} for layer in weights]
    h = torch.from_numpy(x).double()
    for i, p in enumerate(leaves):
        a = _f64_aggregate(kind, h, row, col, w, N_M)
        if kind == "gcn":
            h = a @ p["kernel"] + p["bias"]
        else:
            h = torch.cat([h @ p["self_kernel"], a @ p["neighbor_kernel"]], dim=1) + p["bias"]
        if i == 0:
            h = torch.relu(h)
    out = h[torch.from_numpy(seeds).long()]
    (out * torch.from_numpy(g[:, :out.shape[1]]).double()).sum().backward()
    return out.detach().numpy(), [{k: v.grad.numpy() for k, v in p.items()} for p in leaves]


def _layers(tfg, kind, weights):
    if kind == "gcn":
        make = lambda u, act: tfg.layers.GCN(u, activation=act, norm="left")                       # noqa: E731
    else:
        cls = tfg.layers.MeanGraphSage if kind == "mean" else tfg.layers.SumGraphSage
        make = lambda u, act: cls(u, activation=act, concat=True)                                     # noqa: E731
    units = [w["bias"].shape[0] for w in weights]
    layers = [make(units[0], tfg.relu).trainable(True), make(units[1], None).trainable(True)]
    return layers


def _weights(kind, rng):
    def glorot(a, b):
        lim = np.sqrt(6.0 / (a + b))
        return rng.uniform(-lim, lim, (a, b)).astype(np.float32)
    if kind == "gcn":                              # units > F in both layers: the layer aggregates first (the fused launch)
        dims = [(F_M, 16), (16, 20)]
        return [{"kernel": glorot(a, b), "bias": (rng.standard_normal(b) * 0.1).astype(np.float32)} for a, b in dims]
    dims = [(F_M, 16), (16, 8)]
    return [{"self_kernel": glorot(a, u // 2), "neighbor_kernel": glorot(a, u // 2),
             "bias": (rng.standard_normal(u) * 0.1).astype(np.float32)} for a, u in dims]


def _run_on_blocks(tfg, kind, weights, world_m, count_builds=None):
    ei, ew, x, seeds, g = world_m
    dev = tfg._lib.device()
    sampler = tfg.utils.RandomNeighborSampler(torch.from_numpy(ei).to(dev), torch.from_numpy(ew).to(dev))
    mb = sampler.sample_blocks(seeds, [150, 150], seed=9)          # at the largest degree: every neighbour is kept
    layers = _layers(tfg, kind, weights)
    h = mb.gather(torch.from_numpy(x).to(dev))
    for layer, w in zip(layers, weights):
        layer._maybe_build([torch.empty(1, next(iter(w.values())).shape[0])])      # weights of the layer's own input width
        layer.set_weights(**w)
    if count_builds is not None:
        count_builds["n"] = 0
    for layer, b in zip(layers, mb.blocks):
        h = layer([h[:b.num_src], b.edge_index, b.edge_weight], training=True)[:b.num_dst]
    forward_builds = None if count_builds is None else count_builds["n"]
    out = h[:mb.num_seeds]
    (out * torch.from_numpy(g[:, :out.shape[1]]).to(dev)).sum().backward()
    torch.cuda.synchronize()
    grads = [{k: getattr(layer, k).grad.cpu().numpy() for k in w} for layer, w in zip(layers, weights)]
    return out.detach().cpu().numpy(), grads, mb, forward_builds


def _close(got, ref, what):
    """DESIGN.md §5's bar for float32 layers against float64: 1e-5 of the tensor's largest reference magnitude, every entry."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    print("{:<28s} max|err| = {:.3e}   bar = {:.3e}".format(what, err, 1e-5 * scale))
    assert scale > 0 and err <= 1e-5 * scale, "{}: max|err| {:.3e} > 1e-5 * {:.3e}".format(what, err, scale)


@pytest.mark.parametrize("kind", ["mean", "sum", "gcn"])
def test_two_layers_on_the_blocks_equal_the_full_graph_in_float64(tfg, kind):
    world_m = _model_world(tfg)
    weights = _weights(kind, np.random.Generator(np.random.PCG64(31)))
    ei, ew, x, seeds, g = world_m
    ref_out, ref_grads = _f64_model(kind, x, ei, ew, weights, seeds, g)
    out, grads, mb, _ = _run_on_blocks(tfg, kind, weights, world_m)
    assert mb.blocks[-1].num_dst == 32 and mb.blocks[0].num_src == mb.node_index.numel() > 32
    _close(out, ref_out, kind + " out")
    for i, (got, ref) in enumerate(zip(grads, ref_grads)):
        assert sorted(got) == sorted(ref)
        for k in sorted(ref):
            _close(got[k], ref[k], "{} layer {} d/d{}".format(kind, i, k))


# ---- 5. hand-off --------------------------------------------------------------------------------------------------------
def test_the_layers_use_the_attached_plans(tfg, monkeypatch):
    from tf_geometric_amd import plan as P
    count = {"n": 0}
    real = P.CsrPlan.build

    def counted(*a, **kw):
        count["n"] += 1
        return real(*a, **kw)

    world_m = _model_world(tfg)
    weights = _weights("mean", np.random.Generator(np.random.PCG64(31)))
    monkeypatch.setattr(P.CsrPlan, "build", staticmethod(counted))
    _, _, mb, forward_builds = _run_on_blocks(tfg, "mean", weights, world_m, count_builds=count)
    assert forward_builds == 0, "the forward pass sorted {} edge lists".format(forward_builds)
    assert count["n"] <= len(mb.blocks), "the backward pass built {} plans for {} blocks".format(count["n"], len(mb.blocks))
