# coding=utf-8
"""The fused input hop on the GPU (include/tfgx_samplereduce.h, RandomNeighborSampler.sample_reduce,
sample_blocks(fuse_input_hop=True), MeanGraphSage / SumGraphSage.combine).

One graph serves the kernel tests: 450 nodes built like the one of tests/test_gpu_nbrblock.py (shuffled edge order, random
weights in [0.25, 2], self-loops, duplicate edges, a sink whose id is above every row id) with in-degrees 0, 1, 4, 5, 6, 20, 33,
50, 64, 65, 100 and a hub of 5000, so that the k values below reach every branch of both per-row sampler bodies THROUGH the fused
kernel: k = 5 Floyd (d >= 6) and keep-all; k = 32 / 33 around d = 33; k = 40 lane selection at d = 50 and 64, wave strata at
d = 65, 100, 5000; k = 70 and 128 m > 64, keep-all on a wave at d = 100; k = 8 / 70 with padding: replacement on a lane and on a
wave; k = 0.

  1. Values: float64 numpy over the lists the EXISTING sample_rows returns for the same arguments, at the bar of
     tests/test_gpu_fuzz_forward.py for sums, 1e-5 * sqrt(max column sum of |messages|); counts; NaN-filled surroundings.
  2. Bit identities: run to run, a node's row in two row lists, w = NULL against a sampler of unit weights.
  3. Routes: k = MAX_DRAWS fused, MAX_DRAWS + 1 composed, both at the bar; an x that requires grad is composed and carries d/dx.
  4. Refusals.
  5. The minibatch contract of sample_blocks(fuse_input_hop=True) against the unfused call.
  6. Layers: combine == call, and two layers trained through the fused minibatch equal the whole graph in float64.
"""
import warnings

import numpy as np
import pytest
import torch

from conftest import assert_parity
import f64_layers

pytestmark = pytest.mark.gpu

N_NODES, SINK, ISOLATED, HUB = 450, 449, 0, 11
DEGREES = {0: 0, 1: 1, 2: 4, 3: 5, 4: 6, 5: 20, 6: 33, 7: 50, 8: 64, 9: 65, 10: 100, 11: 5000}
F_MAX = 256


def _graph():
    rng = np.random.Generator(np.random.PCG64(2024))
    n_rows = N_NODES - 1                           # rows 0 .. 448; node 449 only ever appears as a neighbour
    rows, cols = [], []
    for r in range(n_rows):
        d = DEGREES.get(r, int(rng.integers(8, 28)))
        rows.append(np.full(d, r))
        cols.append(rng.integers(0, n_rows, d))    # with repeats: duplicate edges happen
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    for r in (3, 6, 7, 10, 11, 50, 51):            # self-loops
        cols[np.nonzero(rows == r)[0][0]] = r
    for r in (2, 5, 9, 11, 60, 448):               # the sink as a neighbour
        cols[np.nonzero(rows == r)[0][-1]] = SINK
    order = rng.permutation(rows.shape[0])
    ei = np.stack([rows[order], cols[order]]).astype(np.int32)
    ew = rng.uniform(0.25, 2.0, ei.shape[1]).astype(np.float32)
    x = rng.standard_normal((N_NODES, F_MAX)).astype(np.float32)
    return ei, ew, x


@pytest.fixture(scope="module")
def world(tfg):
    ei, ew, x = _graph()
    dev = tfg._lib.device()
    ei_t, ew_t = torch.from_numpy(ei).to(dev), torch.from_numpy(ew).to(dev)
    deg = np.bincount(ei[0], minlength=N_NODES)
    assert all(deg[r] == d for r, d in DEGREES.items()) and deg[SINK] == 0 and ei[1].max() == SINK and ei[0].max() == SINK - 1
    others = np.delete(deg, list(DEGREES) + [SINK])
    assert others.min() >= 8 and others.max() <= 27
    return {"ei": ei_t, "ew": ew_t, "x": x, "dev": dev, "sampler": tfg.utils.RandomNeighborSampler(ei_t, ew_t), "lists": {}}


def _row_lists():
    rng = np.random.Generator(np.random.PCG64(5))
    subset = rng.permutation(N_NODES)[:150]
    if HUB not in subset:
        subset[0] = HUB
    return {"all": np.arange(N_NODES), "shuffled subset": subset,
            "repeated id": np.asarray([10, HUB, 3, 10, SINK, HUB, 6, 10, 9, 8, 7]),
            "isolated and sink": np.asarray([SINK, ISOLATED, SINK, ISOLATED]), "empty": np.zeros(0, np.int64)}


ROW_LISTS = _row_lists()


def _lists(world, name, k, padding, seed):
    """(row position, neighbour id, weight) of the EXISTING sample_rows for a named row list: computed once, never changed."""
    key = (name, k, padding, seed)
    if key not in world["lists"]:
        ei, ew = world["sampler"].sample_rows(ROW_LISTS[name], k=k, padding=padding, seed=seed)
        world["lists"][key] = (ei[0].cpu().numpy().astype(np.int64), ei[1].cpu().numpy().astype(np.int64), ew.cpu().numpy())
    return world["lists"][key]


def _expected(pos, col, w, x, n_rows, op):
    """(float64 reduction, counts, the sqrt-bar's scale) of a list grouped by row position."""
    msg = x[col].astype(np.float64) * w[:, None].astype(np.float64)
    cnt = np.bincount(pos, minlength=n_rows)
    ref = np.zeros((n_rows, x.shape[1]))
    if msg.shape[0]:
        assert (pos[1:] >= pos[:-1]).all()
        starts = (np.cumsum(cnt) - cnt)[cnt > 0]
        ref[cnt > 0] = np.add.reduceat(msg, starts, axis=0)
    if op == "mean":
        ref /= np.maximum(cnt, 1)[:, None]
    return ref, cnt, max(1.0, float(np.abs(msg).sum(0).max()) if msg.shape[0] else 1.0)


def _check(got, ref, scale, what):
    got = got.cpu().numpy()
    assert np.isfinite(got).all(), what + ": unwritten elements"
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    print("{:<70s} max|err| = {:.3e}   bar = {:.3e}".format(what, err, 1e-5 * scale ** 0.5))
    assert_parity(got, ref.astype(np.float32), tol=1e-5 * scale ** 0.5, what=what)


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _x_block(world, F, ox, ld):
    """x[:, :F] as the column block [ox, ox + F) of a NaN-filled buffer whose rows are ld floats apart."""
    wide = _nan((N_NODES, ld), world["dev"])
    wide[:, ox:ox + F] = torch.from_numpy(world["x"][:, :F]).to(world["dev"])
    return wide[:, ox:ox + F]


# width classes of the kernel: the scalar-column fallback (F < 4, a row stride that is no multiple of 4 floats, a start that is
# only 4-byte aligned), 16-byte loads throughout (F % 4 == 0), 16-byte loads with a scalar remainder (F % 4 != 0).
# (F, column offset of x in its buffer, row stride of that buffer, column offset of out, row stride of out's buffer)
SCALAR = [(1, 4, 12, 3, 7), (3, 4, 8, 4, 8), (100, 1, 108, 4, 108), (64, 4, 73, 1, 70)]
VECTOR = [(64, 4, 72, 4, 72), (100, 4, 112, 3, 111), (256, 8, 272, 4, 264)]
REMAINDER = [(130, 4, 140, 4, 136), (130, 8, 144, 1, 135)]
K_CASES = [(5, False), (32, False), (33, False), (40, False), (70, False), (128, False), (8, True), (70, True), (0, False)]


def _widths_for(i):
    """One width of every class for the i-th k: over the k values each width is met, and every k meets every class."""
    return [SCALAR[i % len(SCALAR)], VECTOR[i % len(VECTOR)], REMAINDER[i % len(REMAINDER)]]


def test_the_trimmed_product_covers_every_width():
    seen = {w[0] for i in range(len(K_CASES)) for w in _widths_for(i)}
    assert seen == {1, 3, 64, 100, 130, 256}
    assert {w for i in range(len(K_CASES)) for w in _widths_for(i)} == set(SCALAR + VECTOR + REMAINDER)


# ---- 1. values ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(K_CASES)), ids=["k={}{}".format(k, "-padding" if p else "") for k, p in K_CASES])
def test_values_against_the_lists_of_sample_rows(tfg, world, i):
    from tf_geometric_amd.utils import minibatch as M
    k, padding = K_CASES[i]
    s, dev = world["sampler"], world["dev"]
    for F, ox, ldx, oo, ldo in _widths_for(i):
        xb = _x_block(world, F, ox, ldx)
        assert M.sample_reduce_route(k, xb) == "fused"
        for seed in (3, 2 ** 61 + 12345):
            for name, rows in ROW_LISTS.items():
                pos, col, w = _lists(world, name, k, padding, seed)
                for op in ("mean", "sum"):
                    what = "k={} padding={} F={} x@{}/{} out@{}/{} seed={} rows={} {}".format(k, padding, F, ox, ldx, oo, ldo, seed,
                                                                                              name, op)
                    ref, cnt, scale = _expected(pos, col, w, world["x"][:, :F], len(rows), op)
                    wide = _nan((len(rows), ldo), dev)
                    out, count = s.sample_reduce(rows, xb, k, op=op, padding=padding, seed=seed, out=wide[:, oo:oo + F],
                                                 return_count=True)
                    assert out.data_ptr() == wide[:, oo:oo + F].data_ptr() and tuple(out.shape) == (len(rows), F), what
                    _check(out, ref, scale, what)
                    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), cnt), what
                    assert bool(torch.isnan(wide[:, :oo]).all()) and bool(torch.isnan(wide[:, oo + F:]).all()), what
                    if cnt.size:
                        assert bool((out[torch.from_numpy(cnt == 0).to(dev)] == 0).all()), what      # empty rows: zeros
    # the branches the graph was built for were reached: list lengths of the marked rows in the "all" list
    pos, _, _ = _lists(world, "all", k, padding, 3)
    length = np.bincount(pos, minlength=N_NODES)
    want = {r: (0 if d == 0 else k) if padding else min(d, k) for r, d in DEGREES.items()}
    assert all(length[r] == m for r, m in want.items()) and length[SINK] == 0


# ---- 2. bit identities --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, padding", [(5, False), (40, False), (128, False), (70, True)])
def test_bit_identities(tfg, world, k, padding):
    L = tfg._lib
    s, dev = world["sampler"], world["dev"]
    for F in (3, 100, 130):
        x = torch.from_numpy(world["x"][:, :F]).to(dev).contiguous()
        for op in ("mean", "sum"):
            kw = dict(op=op, padding=padding, seed=41)
            full = s.sample_reduce(ROW_LISTS["all"], x, k, **kw)
            assert torch.equal(full, s.sample_reduce(ROW_LISTS["all"], x, k, **kw))                    # run to run
            # a node's row does not depend on the list it is in (position, neighbours in the tile, repeats)
            for name in ("shuffled subset", "repeated id", "isolated and sink"):
                rows = ROW_LISTS[name]
                assert torch.equal(s.sample_reduce(rows, x, k, **kw), full[torch.from_numpy(rows).to(dev)]), (name, F, op)
            one = s.sample_reduce([HUB], x, k, **kw)
            assert torch.equal(one[0], full[HUB])
    # w = NULL is a graph of unit weights
    ones = tfg.utils.RandomNeighborSampler(world["ei"])
    x = torch.from_numpy(world["x"][:, :100]).to(dev).contiguous()
    want = ones.sample_reduce(ROW_LISTS["all"], x, k, op="sum", padding=padding, seed=41)
    st = ones._nbrblock
    rows = torch.arange(N_NODES, dtype=torch.int32, device=dev)
    out, flag = _nan((N_NODES, 100), dev), torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(L.load_library().tfgx_samplereduce_f32(
        L.ptr(st.row_ptr), L.ptr(ones.plan.col), None, st.n_nodes, L.ptr(rows), N_NODES, k, 1 if padding else 0, 41, L.ptr(x), 100,
        100, L.SUM, L.ptr(out), 100, None, L.ptr(flag), L.stream_ptr()), "tfgx_samplereduce_f32")
    assert torch.equal(out, want) and int(flag.item()) == 0


# ---- 3. routes ----------------------------------------------------------------------------------------------------------
def test_the_two_routes_meet_at_the_draw_limit(tfg, world):
    from tf_geometric_amd.utils import minibatch as M
    s, dev = world["sampler"], world["dev"]
    limit = tfg._lib.SAMPLEREDUCE_MAX_DRAWS
    x = torch.from_numpy(world["x"][:, :12]).to(dev).contiguous()
    for k, route in ((limit, "fused"), (limit + 1, "composed")):
        assert M.sample_reduce_route(k, x) == route
        for name, padding in (("all", False), ("repeated id", True)):
            pos, col, w = _lists(world, name, k, padding, 3)
            for op in ("mean", "sum"):
                ref, cnt, scale = _expected(pos, col, w, world["x"][:, :12], len(ROW_LISTS[name]), op)
                got, count = s.sample_reduce(ROW_LISTS[name], x, k, op=op, padding=padding, seed=3, return_count=True)
                _check(got, ref, scale, "{} k={} {} {}".format(route, k, name, op))
                assert np.array_equal(count.cpu().numpy(), cnt)
        assert np.bincount(_lists(world, "all", k, False, 3)[0], minlength=N_NODES)[HUB] == k


@pytest.mark.parametrize("op", ["mean", "sum"])
def test_an_x_that_requires_grad_takes_the_composed_route_and_carries_its_gradient(tfg, world, op):
    from tf_geometric_amd.utils import minibatch as M
    s, dev = world["sampler"], world["dev"]
    F, k, rows = 12, 40, ROW_LISTS["shuffled subset"]
    x = torch.from_numpy(world["x"][:, :F]).to(dev).contiguous().requires_grad_(True)
    assert M.sample_reduce_route(k, x) == "composed" and M.sample_reduce_route(k, x.detach()) == "fused"
    with torch.no_grad():
        assert M.sample_reduce_route(k, x) == "fused"
    g = np.random.Generator(np.random.PCG64(8)).standard_normal((len(rows), F)).astype(np.float32)
    out = s.sample_reduce(rows, x, k, op=op, seed=3)
    (out * torch.from_numpy(g).to(dev)).sum().backward()
    # the restated sum in float64, differentiated by torch
    pos, col, w = _lists(world, "shuffled subset", k, False, 3)
    x64 = torch.from_numpy(world["x"][:, :F]).double().requires_grad_(True)
    msg = x64[torch.from_numpy(col)] * torch.from_numpy(w).double()[:, None]
    ref = torch.zeros(len(rows), F, dtype=torch.float64).index_add(0, torch.from_numpy(pos), msg)
    cnt = np.bincount(pos, minlength=len(rows))
    if op == "mean":
        ref = ref / torch.from_numpy(np.maximum(cnt, 1)).double()[:, None]
    (ref * torch.from_numpy(g).double()).sum().backward()
    _check(out.detach(), ref.detach().numpy(), float(np.abs(msg.detach().numpy()).sum(0).max()), "composed forward " + op)
    # d/dx[c] sums w * g[row] over the occurrences of c: the bar's scale is the largest such column sum of magnitudes
    back = np.abs(g[pos] * w[:, None])
    per_node = np.zeros((N_NODES, F))
    np.add.at(per_node, col, back)
    _check(x.grad, x64.grad.numpy(), max(1.0, float(per_node.max())), "composed d/dx " + op)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(tfg, world, monkeypatch):
    s, dev = world["sampler"], world["dev"]
    x = torch.from_numpy(world["x"][:, :8]).to(dev).contiguous()
    for rows in ([1, N_NODES], [-1, 2], np.asarray([5, 2 ** 40]), torch.tensor([3, N_NODES], dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"outside \[0, 450\)"):
            s.sample_reduce(rows, x, 5, seed=1)
    with pytest.raises(ValueError, match="449 rows but the sampler's graph has 450 nodes"):
        s.sample_reduce([1, 2], x[:N_NODES - 1], 5, seed=1)
    with pytest.raises(ValueError, match="k=None"):
        s.sample_reduce([1, 2], x, k=None, seed=1)
    with pytest.raises(ValueError, match="ratio="):
        s.sample_reduce([1, 2], x, ratio=0.5, seed=1)
    from tf_geometric_amd.plan import HalfRows
    with pytest.raises(TypeError, match="HalfRows"):
        s.sample_reduce([1, 2], HalfRows.from_dense(x, torch.bfloat16), 5, seed=1)
    with pytest.raises(TypeError, match="float32"):
        s.sample_reduce([1, 2], x.double(), 5, seed=1)
    with pytest.raises(ValueError, match="out must be"):
        s.sample_reduce([1, 2], x, 5, seed=1, out=torch.empty(3, 8, device=dev))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="hipGraph capture"):
        s.sample_reduce([1, 2], x, 5, seed=1)


# ---- 5. the minibatch contract ------------------------------------------------------------------------------------------
SEEDS = [HUB, 17, ISOLATED, SINK, 10, 448, 5, 123, 9]


def _sync_warnings(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            result = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return result, [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]


@pytest.mark.parametrize("padding", [False, True], ids=["", "padding"])
@pytest.mark.parametrize("fanouts", [[5, 5], [40, 5], [8], [5, 5, 5]], ids=str)
def test_the_fused_minibatch_is_the_unfused_one_without_its_input_hop(tfg, world, fanouts, padding):
    L = tfg._lib
    s, dev = world["sampler"], world["dev"]
    n_layers = len(fanouts)
    seeds = torch.tensor(SEEDS, dtype=torch.int32, device=dev)
    unfused = s.sample_blocks(seeds, fanouts, padding=padding, seed=77)
    s.sample_blocks(seeds, fanouts, padding=padding, seed=77, fuse_input_hop=True)        # warm: allocator, first launches
    fused, reads = _sync_warnings(lambda: s.sample_blocks(seeds, fanouts, padding=padding, seed=77, fuse_input_hop=True))
    assert len(reads) == n_layers == fused.num_host_syncs == unfused.num_host_syncs - 1, reads
    assert int((s._nbrblock.table != L.NBRBLOCK_EMPTY).sum()) == 0
    # the blocks of layers 1 .. L-1 and the nodes known after the inner hops, bit for bit
    assert unfused.input_hop is None and len(unfused.blocks) == n_layers and len(fused.blocks) == n_layers - 1
    for a, b in zip(fused.blocks, unfused.blocks[1:]):
        assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.edge_weight, b.edge_weight)
        assert (a.num_dst, a.num_src) == (b.num_dst, b.num_src)
    n_inner = unfused.blocks[0].num_dst
    assert fused.node_index.dtype == torch.int32 and torch.equal(fused.node_index, unfused.node_index[:n_inner])
    assert fused.num_seeds == len(SEEDS) and fused.hop_seeds == unfused.hop_seeds
    assert fused.input_hop == (fanouts[0], padding, unfused.hop_seeds[-1])
    if n_layers == 1:
        assert fused.blocks == [] and torch.equal(fused.node_index, seeds)
    # the input hop: the reduction of the unfused call's gathered rows over its blocks[0]
    b0 = unfused.blocks[0]
    pos, vcol = (t.cpu().numpy().astype(np.int64) for t in b0.edge_index)
    for F in (3, 100):
        x = torch.from_numpy(world["x"][:, :F]).to(dev).contiguous()
        gathered = unfused.gather(x).cpu().numpy()
        assert torch.equal(fused.gather(x), unfused.gather(x)[:n_inner])
        for op in ("mean", "sum"):
            ref, _, scale = _expected(pos, vcol, b0.edge_weight.cpu().numpy(), gathered, n_inner, op)
            fused.input_aggregate(x, op)                                                      # warm
            got, reads = _sync_warnings(lambda: fused.input_aggregate(x, op))
            assert reads == [], reads
            assert tuple(got.shape) == (n_inner, F)
            _check(got, ref, scale, "input_aggregate {} padding={} F={} {}".format(fanouts, padding, F, op))
            assert torch.equal(got, s.sample_reduce(fused.node_index, x, fanouts[0], op=op, padding=padding, seed=fused.hop_seeds[-1]))


def test_the_table_is_clean_after_a_refused_fused_call(tfg, world):
    L = tfg._lib
    s = tfg.utils.RandomNeighborSampler(world["ei"], world["ew"])
    want = s.sample_blocks(SEEDS, [5, 3], seed=1, fuse_input_hop=True)
    for bad, word in (([3, HUB, 9, 3], "repeat"), ([3, N_NODES, 9], r"outside \[0, 450\)"), ([3, -1, 9], r"outside \[0, 450\)")):
        for fanouts in ([5, 3], [5]):
            with pytest.raises(ValueError, match=word):
                s.sample_blocks(bad, fanouts, seed=1, fuse_input_hop=True)
            again = s.sample_blocks(SEEDS, [5, 3], seed=1, fuse_input_hop=True)
            assert torch.equal(again.node_index, want.node_index) and torch.equal(again.blocks[0].edge_index, want.blocks[0].edge_index)
            assert int((s._nbrblock.table != L.NBRBLOCK_EMPTY).sum()) == 0


# ---- 6. layers ----------------------------------------------------------------------------------------------------------
N_M, F_M = 300, 12


def _model_world():
    rng = np.random.Generator(np.random.PCG64(21))
    deg = rng.integers(0, 13, N_M - 1)             # rows 0 .. 298, some without neighbours; node 299 is a sink
    deg[40], deg[41] = 40, 33
    rows = np.repeat(np.arange(N_M - 1), deg)
    cols = rng.integers(0, N_M, rows.shape[0])
    order = rng.permutation(rows.shape[0])
    ei = np.stack([rows[order], cols[order]]).astype(np.int32)
    ew = rng.uniform(0.5, 1.5, ei.shape[1]).astype(np.float32)
    x = rng.standard_normal((N_M, F_M)).astype(np.float32)
    seeds = rng.permutation(N_M)[:32]
    if 40 not in seeds:
        seeds[3] = 40
    g = rng.standard_normal((32, 64)).astype(np.float32)
    assert deg.max() == 40 and ei[1].max() == N_M - 1
    return ei, ew, x, seeds, g


def _weights(rng):
    def glorot(a, b):
        lim = np.sqrt(6.0 / (a + b))
        return rng.uniform(-lim, lim, (a, b)).astype(np.float32)
    return [{"self_kernel": glorot(a, u // 2), "neighbor_kernel": glorot(a, u // 2),
             "bias": (rng.standard_normal(u) * 0.1).astype(np.float32)} for a, u in [(F_M, 16), (16, 8)]]


def _f64_model(kind, x, ei, ew, weights, seeds, g):
    """Both layers over the WHOLE graph in float64 on the CPU (segment sums of tests/f64_layers.py over the destination-sorted
    list; nn/conv/graph_sage.py:9-115 written out), read at the seed rows; gradients of sum(out[seeds] * g)."""
    edges = f64_layers.SortedEdges(torch.from_numpy(ei), N_M)
    w = edges.edge_attr(torch.from_numpy(ew).double())
    leaves = [{k: torch.from_numpy(v).double().requires_grad_(True) for k, v in layer.items()} for layer in weights]
    h = torch.from_numpy(x).double()
    for i, p in enumerate(leaves):
        a = edges.seg_sum(w[:, None] * h[edges.col])
        if kind == "mean":
            a = a / edges.lengths.clamp(min=1).double()[:, None]
        h = torch.cat([h @ p["self_kernel"], a @ p["neighbor_kernel"]], dim=1) + p["bias"]
        if i == 0:
            h = torch.relu(h)
    out = h[torch.from_numpy(seeds).long()]
    (out * torch.from_numpy(g[:, :out.shape[1]]).double()).sum().backward()
    return out.detach().numpy(), [{k: v.grad.numpy() for k, v in p.items()} for p in leaves]


def _close(got, ref, what):
    """DESIGN.md §5's bar for float32 layers against float64: 1e-5 of the tensor's largest reference magnitude, every entry."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    print("{:<28s} max|err| = {:.3e}   bar = {:.3e}".format(what, err, 1e-5 * scale))
    assert scale > 0 and err <= 1e-5 * scale, "{}: max|err| {:.3e} > 1e-5 * {:.3e}".format(what, err, scale)


@pytest.mark.parametrize("kind", ["mean", "sum"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "add"])
def test_combine_is_call_on_a_whole_graph(tfg, kind, concat):
    ei, ew, x, _, _ = _model_world()
    dev = tfg._lib.device()
    ei_t, ew_t, x_t = torch.from_numpy(ei).to(dev), torch.from_numpy(ew).to(dev), torch.from_numpy(x).to(dev)
    sampler = tfg.utils.RandomNeighborSampler(ei_t, ew_t)
    agg = sampler.sample_reduce(np.arange(N_M), x_t, 64, op=kind, seed=1)          # k above every degree: every neighbour, in order
    cls = tfg.layers.MeanGraphSage if kind == "mean" else tfg.layers.SumGraphSage
    layer = cls(16, activation=tfg.relu, concat=concat, normalize=True)
    got = layer.combine([x_t, agg])                                                # builds the weights from x's width
    kernels = (layer.self_kernel, layer.neighbor_kernel, layer.bias)
    assert tuple(layer.self_kernel.shape) == (F_M, 8 if concat else 16)
    ref = layer([x_t, ei_t, ew_t])
    assert all(a is b for a, b in zip(kernels, (layer.self_kernel, layer.neighbor_kernel, layer.bias)))      # shared with call
    assert tuple(got.shape) == tuple(ref.shape) == (N_M, 16)
    _close(got.cpu().numpy(), ref.cpu().numpy(), "{} combine vs call".format(kind))
    fn = tfg.nn.graph_sage_combine(x_t, agg, layer.self_kernel, layer.neighbor_kernel, bias=layer.bias, activation=tfg.relu,
                                   concat=concat, normalize=True)
    assert torch.equal(fn, got)
    with pytest.raises(ValueError, match="must both be"):
        tfg.nn.graph_sage_combine(x_t, agg[:, :5], layer.self_kernel, layer.neighbor_kernel)


@pytest.mark.parametrize("kind", ["mean", "sum"])
def test_two_layers_through_the_fused_minibatch_equal_the_full_graph_in_float64(tfg, kind):
    ei, ew, x, seeds, g = _model_world()
    weights = _weights(np.random.Generator(np.random.PCG64(31)))
    ref_out, ref_grads = _f64_model(kind, x, ei, ew, weights, seeds, g)
    dev = tfg._lib.device()
    sampler = tfg.utils.RandomNeighborSampler(torch.from_numpy(ei).to(dev), torch.from_numpy(ew).to(dev))
    mb = sampler.sample_blocks(seeds, [64, 64], seed=9, fuse_input_hop=True)       # above the largest degree: every neighbour
    assert len(mb.blocks) == 1 and mb.blocks[0].num_dst == 32 and mb.node_index.numel() == mb.blocks[0].num_src > 32
    cls = tfg.layers.MeanGraphSage if kind == "mean" else tfg.layers.SumGraphSage
    layers = [cls(16, activation=tfg.relu, concat=True).trainable(True), cls(8, activation=None, concat=True).trainable(True)]
    for layer, w in zip(layers, weights):
        layer._maybe_build([torch.empty(1, w["self_kernel"].shape[0])])
        layer.set_weights(**w)
    x_t = torch.from_numpy(x).to(dev)
    h = layers[0].combine([mb.gather(x_t), mb.input_aggregate(x_t, kind)], training=True)
    for layer, b in zip(layers[1:], mb.blocks):
        h = layer([h[:b.num_src], b.edge_index, b.edge_weight], training=True)[:b.num_dst]
    out = h[:mb.num_seeds]
    (out * torch.from_numpy(g[:, :out.shape[1]]).to(dev)).sum().backward()
    torch.cuda.synchronize()
    _close(out.detach().cpu().numpy(), ref_out, kind + " out")
    for i, (layer, ref) in enumerate(zip(layers, ref_grads)):
        for name in sorted(ref):
            _close(getattr(layer, name).grad.cpu().numpy(), ref[name], "{} layer {} d/d{}".format(kind, i, name))


def test_the_demo_trains_with_the_fused_input_hop():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("demo_graph_sage_minibatch",
                                                  os.path.join(ROOT, "examples", "demo_graph_sage_minibatch.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    acc, loss = demo.main(epochs=3, batch=512, num_nodes=4000, quiet=True, fuse_input_hop=True)
    print("fused demo: test accuracy {:.3f}, last loss {:.3f}".format(acc, loss))
    assert np.isfinite(loss) and acc > 1.0 / 6        # six planted classes: better than chance after three short epochs
