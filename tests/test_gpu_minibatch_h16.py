# coding=utf-8
"""The minibatch route over a 16-bit feature table on the GPU (include/tfgx_minibatch_h16.h; prepare_half_features(...,
minibatch=True) through RandomNeighborSampler.sample_reduce, SampledMinibatch / StaticMinibatch.gather and .input_aggregate).

The contract is a bit contract, so every comparison is torch.equal against the float32 entry point on h.float() — no tolerance.

One graph of 320 nodes: a hub with 300 neighbours, rows of 0, 1, 31, 32, 33, 63, 64, 65 and 130 neighbours (around the lane / wave
branches of the sampler bodies and the k values below), the rest with 0 .. 20, random weights and a twin sampler without weights;
node 319, the table's last row, is both a destination and a neighbour.  Tables: one float32 matrix of finite values whose columns
cycle through scales that reach fp16 subnormals (3e-6) and large bf16 magnitudes (1e30; 1e3 for fp16, which has no such range),
quantised to both types at F in {1, 7, 8, 9, 100, 257} on the friendly stride and on roundup8(F); the columns [F, ld) of every
row are overwritten with NaN before use: nothing of them may reach the output.

  1. sample_reduce: k in {0, 1, 5, 32, 33, 64, 65, 256}, both paddings, both ops over 71 rows (a prime: no multiple of any tile)
     with repeats, empty rows, the hub and node 319: out, out_count, and an out= view into a wider buffer of sentinels.  k = 257 and
     a table whose source requires grad take the composed route and equal the float32 composed route; d/dx reaches the source.
  2. The row-id ValueErrors of the float32 route.
  3. gather on both minibatch classes, the static one with dead seeds first, in the middle and last; one direct call into a
     sentinel-filled buffer.
  4. A two-layer MeanGraphSage step through sample_blocks(fuse_input_hop=True): loss and every weight gradient.
  5. Static: no host read under torch.cuda.set_sync_debug_mode("error"); three replays of a captured training step.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, HUB, LAST = 320, 5, 319
DEGREES = {HUB: 300, 10: 0, 11: 1, 12: 31, 13: 32, 14: 33, 15: 63, 16: 64, 17: 65, 18: 130, LAST: 7}
WIDTHS = [1, 7, 8, 9, 100, 257]
DTYPES = [torch.bfloat16, torch.float16]
K_VALUES = [0, 1, 5, 32, 33, 64, 65, 256]
SENTINEL = -7.5


def _graph():
    rng = np.random.Generator(np.random.PCG64(320))
    rows, cols = [], []
    for r in range(N):
        d = DEGREES.get(r, int(rng.integers(0, 21)))
        rows.append(np.full(d, r))
        cols.append(rng.integers(0, N, d))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    for r in (HUB, 12, 18, 100):                      # the table's last row as a neighbour
        cols[np.nonzero(rows == r)[0][0]] = LAST
    order = rng.permutation(rows.shape[0])
    ei = np.stack([rows[order], cols[order]]).astype(np.int32)
    ew = rng.uniform(0.25, 2.0, ei.shape[1]).astype(np.float32)
    return ei, ew


def _values(dtype):
    """[N, 257] finite float32 values; column j is scaled by one of three magnitudes, the smallest inside the fp16 subnormals."""
    rng = np.random.Generator(np.random.PCG64(16))
    scales = np.asarray([3e-6, 1.0, 1e30 if dtype == torch.bfloat16 else 1e3], dtype=np.float32)
    x = rng.standard_normal((N, max(WIDTHS))).astype(np.float32) * scales[np.arange(max(WIDTHS)) % 3][None, :]
    assert np.isfinite(x).all()
    return x


def _rows():
    rng = np.random.Generator(np.random.PCG64(71))
    rows = rng.integers(0, N, 71)
    rows[:12] = [HUB, LAST, 10, 11, 12, 13, 14, 15, 16, 17, 18, HUB]       # the marked rows, the hub twice
    rows[40], rows[70] = 10, LAST                                          # an empty row again, node 319 as the last row
    return rows


@pytest.fixture(scope="module")
def world(tfg):
    ei, ew = _graph()
    dev = tfg._lib.device()
    ei_t, ew_t = torch.from_numpy(ei).to(dev), torch.from_numpy(ew).to(dev)
    deg = np.bincount(ei[0], minlength=N)
    assert all(deg[r] == d for r, d in DEGREES.items()) and deg.max() == 300 and LAST in ei[1] and ei[0].max() == LAST
    assert np.delete(deg, list(DEGREES)).max() <= 20
    return {"dev": dev, "ei": ei_t, "ew": ew_t, "weighted": tfg.utils.RandomNeighborSampler(ei_t, ew_t),
            "unit": tfg.utils.RandomNeighborSampler(ei_t), "rows": torch.from_numpy(_rows()).to(dev), "tables": {}, "ref": {}}


def _strides(tfg, F):
    from tf_geometric_amd.plan import h16_friendly_ld
    return [h16_friendly_ld(F), (F + 7) // 8 * 8]


def _table(tfg, world, dtype, F, ld):
    """(the declared HalfRows on stride ld with NaN pad columns, its widened float32 table): made once, never changed."""
    key = (dtype, F, ld)
    if key not in world["tables"]:
        x = torch.from_numpy(_values(dtype)[:, :F]).to(world["dev"])
        h = tfg.prepare_half_features(x, dtype, ld=ld, minibatch=True)
        assert h.minibatch and h.ld == ld and tuple(h.table.shape) == (N, ld) and h.shape == (N, F)
        xf = h.float()
        h.table[:, F:] = float("nan")
        assert torch.equal(h.float(), xf) and bool(torch.isfinite(xf).all())
        if ld > F:
            assert bool(torch.isnan(h.table[:, F:].float()).all())
        if dtype == torch.float16 and F >= 7:      # the quantised table holds fp16 subnormals; the bf16 one large magnitudes
            assert bool(((xf != 0) & (xf.abs() < 6.0e-5)).any())
        if dtype == torch.bfloat16 and F >= 7:
            assert float(xf.abs().max()) > 1e30
        world["tables"][key] = (h, xf)
    return world["tables"][key]


def _reference(world, name, xf, key, k, padding, op):
    """tfgx_samplereduce_f32 on the widened table: computed once per case and shared by both strides."""
    key = (name,) + key + (k, padding, op)
    if key not in world["ref"]:
        world["ref"][key] = world[name].sample_reduce(world["rows"], xf, k, op=op, padding=padding, seed=77, return_count=True)
    return world["ref"][key]


# ---- 1. sample_reduce ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_sample_reduce_returns_the_float32_bits(tfg, world, dtype, F):
    from tf_geometric_amd.utils import minibatch as M
    dev, rows = world["dev"], world["rows"]
    n_rows = int(rows.shape[0])
    assert n_rows == 71
    for i, ld in enumerate(_strides(tfg, F)):
        h, xf = _table(tfg, world, dtype, F, ld)
        # the out= view: 16-byte aligned rows and start on the first stride (16-byte stores), neither on the second (per column)
        oo, ldo = (4, (F + 3) // 4 * 4 + 8) if i == 0 else (3, F + 5)
        for name, ks in (("weighted", K_VALUES), ("unit", [5, 65])):
            s = world[name]
            for k in ks:
                assert M.sample_reduce_route(k, h) == "fused"
                for padding in (False, True):
                    for op in ("mean", "sum"):
                        what = "{} F={} ld={} {} k={} padding={} {}".format(dtype, F, ld, name, k, padding, op)
                        want, want_count = _reference(world, name, xf, (dtype, F), k, padding, op)
                        got, count = s.sample_reduce(rows, h, k, op=op, padding=padding, seed=77, return_count=True)
                        assert got.dtype == torch.float32 and tuple(got.shape) == (n_rows, F), what
                        assert torch.equal(got, want), what
                        assert count.dtype == torch.int32 and torch.equal(count, want_count), what
                        wide = torch.full((n_rows, ldo), SENTINEL, dtype=torch.float32, device=dev)
                        out = s.sample_reduce(rows, h, k, op=op, padding=padding, seed=77, out=wide[:, oo:oo + F])
                        assert out.data_ptr() == wide[:, oo:oo + F].data_ptr() and torch.equal(out, want), what
                        assert bool((wide[:, :oo] == SENTINEL).all()) and bool((wide[:, oo + F:] == SENTINEL).all()), what
    # the lists were what the graph was built for: the marked rows drew min(d, k) (k under padding) neighbours
    _, count = _reference(world, "weighted", xf, (dtype, F), 65, False, "sum")
    _, padded = _reference(world, "weighted", xf, (dtype, F), 65, True, "sum")
    marked = {int(r): i for i, r in enumerate(_rows()[:12])}
    for r, d in DEGREES.items():
        assert int(count[marked[r]]) == min(d, 65) and int(padded[marked[r]]) == (65 if d > 0 else 0), r


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_the_composed_route_equals_the_float32_composed_route(tfg, world, dtype):
    from tf_geometric_amd.plan import HalfRows
    from tf_geometric_amd.utils import minibatch as M
    s, dev, rows = world["weighted"], world["dev"], world["rows"]
    F = 100
    h, xf = _table(tfg, world, dtype, F, _strides(tfg, F)[0])
    assert M.sample_reduce_route(257, h) == M.sample_reduce_route(257, xf) == "composed"
    for op in ("mean", "sum"):
        for padding in (False, True):
            got, count = s.sample_reduce(rows, h, 257, op=op, padding=padding, seed=5, return_count=True)
            want, want_count = s.sample_reduce(rows, xf, 257, op=op, padding=padding, seed=5, return_count=True)
            assert torch.equal(got, want) and torch.equal(count, want_count), (op, padding)
    # a table whose source requires grad: composed at any k, the float32 composed route's bits, and d/dx reaches the source
    src = xf.to(dtype).requires_grad_(True)                      # exact: xf holds values of that type
    trained = HalfRows.from_tensor(src, minibatch=True)
    x32 = xf.clone().requires_grad_(True)
    assert trained.requires_grad and M.sample_reduce_route(5, trained) == M.sample_reduce_route(5, x32) == "composed"
    g = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).standard_normal((int(rows.shape[0]), F)).astype(np.float32)).to(dev)
    for op in ("mean", "sum"):
        src.grad = x32.grad = None
        got = s.sample_reduce(rows, trained, 5, op=op, seed=5)
        want = s.sample_reduce(rows, x32, 5, op=op, seed=5)
        assert torch.equal(got, want), op
        (got * g).sum().backward()
        (want * g).sum().backward()
        assert src.grad is not None and src.grad.dtype == dtype and tuple(src.grad.shape) == (N, F)
        # the source receives the float32 gradient rounded once to its type: half an ulp of that type, 2^-9 of the value for bf16
        # (8 significand bits) and 2^-12 for fp16 above its subnormals, whose spacing is 2^-24; the bound below takes 2^-8 and 2^-23
        ref = x32.grad
        assert bool((ref != 0).any()) and bool(torch.isfinite(src.grad.float()).all())
        err = (src.grad.float() - ref).abs()
        assert bool((err <= ref.abs() * 2.0 ** -8 + 2.0 ** -23).all()), (op, float(err.max()))


# ---- 2. refusals --------------------------------------------------------------------------------------------------------
def test_the_row_id_refusals_of_the_float32_route(tfg, world):
    s = world["weighted"]
    h, xf = _table(tfg, world, torch.bfloat16, 8, 8)
    for rows in ([1, N], [-1, 2], np.asarray([5, 2 ** 40]), torch.tensor([3, N], dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"outside \[0, 320\)"):
            s.sample_reduce(rows, h, 5, seed=1)
        with pytest.raises(ValueError, match=r"outside \[0, 320\)"):
            s.sample_reduce(rows, h, 257, seed=1)
    short = tfg.prepare_half_features(xf[:N - 1], torch.bfloat16, minibatch=True)
    with pytest.raises(ValueError, match="319 rows but the sampler's graph has 320 nodes"):
        s.sample_reduce([1, 2], short, 5, seed=1)
    mb = s.sample_blocks([1, 2, 3], [5, 3], seed=1, fuse_input_hop=True)
    static = s.sample_blocks_static([1, 2, 3], [5, 3], seed=1, fuse_input_hop=True)
    for call in (lambda: mb.gather(short), lambda: mb.input_aggregate(short), lambda: static.gather(short),
                 lambda: static.input_aggregate(short)):
        with pytest.raises(ValueError, match="319 rows but the sampler's graph has 320 nodes"):
            call()
    undeclared = tfg.prepare_half_features(xf, torch.bfloat16)
    assert not undeclared.minibatch
    for call in (lambda: s.sample_reduce([1, 2], undeclared, 5, seed=1), lambda: mb.gather(undeclared),
                 lambda: static.gather(undeclared), lambda: static.input_aggregate(undeclared)):
        with pytest.raises(TypeError, match="HalfRows"):
            call()
    with pytest.raises(ValueError, match="out must be"):
        s.sample_reduce([1, 2], h, 5, seed=1, out=torch.empty(3, 8, device=world["dev"]))


# ---- 3. gather ----------------------------------------------------------------------------------------------------------
SEEDS = [HUB, 17, 10, LAST, 100, 18, 200, 11]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_gather_on_both_minibatch_classes(tfg, world, dtype):
    L = tfg._lib
    s, dev = world["weighted"], world["dev"]
    mb = s.sample_blocks(SEEDS, [5, 3], seed=9)
    slots = torch.tensor([-1] + SEEDS[:4] + [-1, -1] + SEEDS[4:] + [-1], dtype=torch.int32, device=dev)
    static = s.sample_blocks_static(slots, [5, 3], seed=9)
    dead = static.node_index < 0
    assert bool(dead[0]) and bool(dead[5]) and bool(dead[6]) and bool(dead[len(slots) - 1]) and not bool(dead[1])
    assert int((static.node_index == LAST).sum()) == 1 and int((mb.node_index == LAST).sum()) == 1
    for F in WIDTHS:
        for ld in _strides(tfg, F):
            h, xf = _table(tfg, world, dtype, F, ld)
            got = mb.gather(h)
            assert got.dtype == torch.float32 and torch.equal(got, mb.gather(xf)) and torch.equal(got, xf[mb.node_index.long()])
            got = static.gather(h)
            assert torch.equal(got, static.gather(xf)) and bool((got[dead] == 0).all()) and tuple(got.shape) == (len(dead), F)
            # the entry point itself, into a buffer of sentinels: 16-byte stores (aligned rows) and one store per column
            for oo, ldo in ((4, (F + 3) // 4 * 4 + 8), (3, F + 5)):
                wide = torch.full((len(dead), ldo), SENTINEL, dtype=torch.float32, device=dev)
                view = wide[:, oo:oo + F]
                L.check(L.load_library().tfgx_gather_rows_h16_f32(L.ptr(h.table), h.ld, L.H16_DTYPES[dtype], L.ptr(static.node_index),
                                                                  len(dead), F, L.ptr(view), ldo, L.stream_ptr()), "gather")
                assert torch.equal(view, got), (F, ld, oo)
                assert bool((wide[:, :oo] == SENTINEL).all()) and bool((wide[:, oo + F:] == SENTINEL).all()), (F, ld, oo)


# ---- 4. a training step through the fused dynamic minibatch -------------------------------------------------------------
def _layers(tfg, F, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    layers = [tfg.layers.MeanGraphSage(16, activation=tfg.relu, concat=True).trainable(True),
              tfg.layers.MeanGraphSage(8, activation=None, concat=True).trainable(True)]
    for layer, (a, u) in zip(layers, [(F, 16), (16, 8)]):
        lim = np.sqrt(6.0 / (a + u // 2))
        layer._maybe_build([torch.empty(1, a)])
        layer.set_weights(self_kernel=rng.uniform(-lim, lim, (a, u // 2)).astype(np.float32),
                          neighbor_kernel=rng.uniform(-lim, lim, (a, u // 2)).astype(np.float32),
                          bias=(rng.standard_normal(u) * 0.1).astype(np.float32))
    return layers


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_a_two_layer_step_over_the_table_equals_the_step_over_its_float32_copy(tfg, world, dtype):
    s, dev = world["weighted"], world["dev"]
    F = 100
    h, xf = _table(tfg, world, dtype, F, _strides(tfg, F)[0])
    # columns of magnitude 1 only reach the loss through finite products; the 1e30 columns of the bf16 table would overflow it
    scale = torch.from_numpy((np.arange(F) % 3 == 1).astype(np.float32)).to(dev)
    results = []
    for table in (h, xf):
        layers = _layers(tfg, F, 41)
        mb = s.sample_blocks(SEEDS, [33, 5], seed=13, fuse_input_hop=True)
        assert len(mb.blocks) == 1 and mb.input_hop[0] == 33
        h0 = layers[0].combine([mb.gather(table) * scale, mb.input_aggregate(table, "mean") * scale], training=True)
        b = mb.blocks[0]
        out = layers[1]([h0[:b.num_src], b.edge_index, b.edge_weight], training=True)[:b.num_dst]
        loss = (out[:mb.num_seeds] ** 2).sum()
        loss.backward()
        results.append((loss.detach(), [getattr(layer, n).grad for layer in layers for n in ("self_kernel", "neighbor_kernel", "bias")]))
    (loss_h, grads_h), (loss_f, grads_f) = results
    assert bool(torch.isfinite(loss_h)) and float(loss_h) > 0 and torch.equal(loss_h, loss_f)
    assert len(grads_h) == 6
    for a, b in zip(grads_h, grads_f):
        assert a is not None and bool((a != 0).any()) and torch.equal(a, b)


# ---- 5. static: no host read, and a captured step -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_the_static_route_over_the_table_makes_no_host_read(tfg, world, dtype):
    s, dev = world["weighted"], world["dev"]
    slots = torch.tensor([-1] + SEEDS[:4] + [-1] + SEEDS[4:] + [-1], dtype=torch.int32, device=dev)
    state = torch.full((1,), 900, dtype=torch.int64, device=dev)
    for F in (9, 100):
        h, xf = _table(tfg, world, dtype, F, _strides(tfg, F)[0])

        def run(table):
            mb = s.sample_blocks_static(slots, [33, 5], seed=state, fuse_input_hop=True)
            return mb, mb.gather(table), mb.input_aggregate(table, "mean"), mb.input_aggregate(table, "sum")

        run(h)                                                  # warm: the sampler's state, the allocator, first launches
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            mb, rows, mean, total = run(h)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert mb.num_host_syncs == 0
        _, rows_f, mean_f, total_f = run(xf)
        assert torch.equal(rows, rows_f) and torch.equal(mean, mean_f) and torch.equal(total, total_f)
        dead = mb.node_index < 0
        assert bool(dead[0]) and bool((mean[dead] == 0).all()) and bool((rows[dead] == 0).all()) and bool((total[~dead] != 0).any())
        assert int(mb.flag.item()) == 0
        # bit for bit what the dynamic route gives the same nodes
        live = mb.node_index[~dead]
        k, padding, hop = mb.input_hop
        from tf_geometric_amd.utils.minibatch import hop_seed
        assert torch.equal(mean[~dead], s.sample_reduce(live, h, k, op="mean", padding=padding, seed=hop_seed(900, hop)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_three_replays_of_a_captured_step_equal_those_over_the_float32_copy(tfg, world, dtype):
    s, dev = world["weighted"], world["dev"]
    F = 100
    h, xf = _table(tfg, world, dtype, F, _strides(tfg, F)[0])
    scale = torch.from_numpy((np.arange(F) % 3 == 1).astype(np.float32)).to(dev)
    slots = torch.tensor(SEEDS[:5] + [-1] + SEEDS[5:], dtype=torch.int32, device=dev)
    state = torch.full((1,), 500, dtype=torch.int64, device=dev)
    losses = []
    for table in (h, xf):
        layers = _layers(tfg, F, 43)
        opt = torch.optim.Adam([p for layer in layers for p in layer.parameters()], lr=1e-2, capturable=True)

        def loss_fn():
            mb = s.sample_blocks_static(slots, [33, 5], seed=state, fuse_input_hop=True)
            state.add_(1)
            h0 = layers[0].combine([mb.gather(table) * scale, mb.input_aggregate(table, "mean") * scale], training=True)
            b = mb.blocks[0]
            out = layers[1]([h0[:b.num_src], b.edge_index, b.edge_weight], training=True)[:b.num_dst]
            return ((out[:mb.num_seeds] ** 2).sum(1) * mb.seed_mask).sum()

        step = tfg.CapturedTrainStep(loss_fn, opt)
        state.fill_(500)                                         # the warm-up steps advanced the seed: both start at the same one
        losses.append(torch.stack([step().detach().clone() for _ in range(3)]))
        assert int(state) == 503
    print("captured over the table ", losses[0].tolist())
    print("captured over float32   ", losses[1].tolist())
    assert bool(torch.isfinite(losses[0]).all()) and len(set(losses[0].tolist())) == 3
    assert torch.equal(losses[0], losses[1])
