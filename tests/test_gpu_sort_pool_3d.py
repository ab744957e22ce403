# coding=utf-8
"""tfgx_segment_rows_3d_f32 and what is built on it, on the GPU: utils.convert_x_to_3d, nn.sort_pool_3d, SortPool.pool_3d and the
fixed-shape forms (nn.sort_pool_static, SortPool.pool_static, StaticBatchGraph.to_3d).

The operation only moves values, so every comparison of outputs and of dx is EXACT: against the numpy mirror
(tests/sortpool3d_mirror.py, itself held to the reference's recorded outputs by tests/test_sortpool3d_reference.py), against the
composed route convert_x_to_3d(sort_pool(...)[0], pooled_node_graph_index, k, num_sources=G), and against nn.topk_pool's
selection where keys tie.  The one exception is the model-level float64 check, at the bar of the other model tests: each entry
within 1e-5 of the tensor's largest reference magnitude."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import sortpool3d_cases as sc
from sortpool3d_mirror import (MAX_GRAPH_NODES, TOO_LONG, graph_plan, mirror_backward, mirror_convert_x_to_3d, mirror_rows_3d,
                               mirror_sort_pool_3d)
from test_collate_abi import random_dataset

pytestmark = pytest.mark.gpu

DEV = "cuda"
sys.path.insert(0, os.path.join(ROOT, "examples"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sortpool3d_cases.npz")

# graph sizes: around one wave (64), the 4 keys a thread holds per pass (256 threads: 1024), one and several ranking passes, the cap
BATCHES = {"G=1 n=0": [0], "G=1 n=1": [1], "G=1 n=65": [65], "G=1 n=1025": [1025], "G=1 n=4096": [MAX_GRAPH_NODES],
           "G=9 empty first, middle and last": [0, 3, 64, 0, 257, 2, 1023, 63, 0],
           "G=9 every boundary": [1025, 256, 65, 1, MAX_GRAPH_NODES, 2, 3, 64, 63]}
KS = (1, 2, 3, 30, 64, 5000)            # 5000 exceeds every graph
FS = (1, 3, 4, 5, 32, 97, 128, 257)
# every k at two widths (one on the 16-byte path, one not), every F at k = 30, and the largest of both once
COMBOS = [(k, F) for k in KS for F in (5, 128)] + [(30, F) for F in FS if F not in (5, 128)] + [(5000, 257)]


def _eq(got, ref, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, "{}: {} {} vs {} {}".format(what, got.shape, got.dtype, ref.shape, ref.dtype)
    if got.dtype.kind == "f":           # bits, so that NaNs compare too
        got, ref = got.view(np.int32), ref.view(np.int32)
    assert np.array_equal(got, ref), "{}: {} entries differ".format(what, int((got != ref).sum()))


def _batch(sizes, F, seed, interleave, distinct=True):
    """x [n, F] float32 (sort columns without ties when `distinct`), node_graph_index [n], edge_index [2, e] (a few edges inside
    every graph: the composed route pools them), as numpy."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gid = np.concatenate([np.full(s, g, dtype=np.int32) for g, s in enumerate(sizes)] + [np.zeros(0, np.int32)])
    if interleave:
        gid = gid[rng.permutation(gid.size)]
    n = gid.size
    x = rng.standard_normal((n, F)).astype(np.float32)
    if distinct:
        for c in {0, F // 2, F - 1}:
            x[:, c] = (rng.permutation(n) - n // 2).astype(np.float32) * 0.25
    edges = [np.zeros((2, 0), np.int32)]
    for g in range(len(sizes)):
        nodes = np.flatnonzero(gid == g)
        if nodes.size:
            edges.append(rng.choice(nodes, (2, min(nodes.size, 40))).astype(np.int32))
    return x, gid, np.concatenate(edges, axis=1)


def _dev(x, offset=0, pad=0):
    """x on the device; with offset / pad a column block of a wider buffer (ldx != F; offset 1: the base is not 16-byte aligned)."""
    t = torch.from_numpy(x).to(DEV)
    if not (offset or pad):
        return t
    wide = torch.full((x.shape[0], x.shape[1] + offset + pad), 7.0, device=DEV)
    wide[:, offset:offset + x.shape[1]] = t
    return wide[:, offset:offset + x.shape[1]]


def _raw(tfg, x, seg_ptr, seg_node, G, k, sort_col=None):
    """The entry point itself: (out, slot_node, node_slot, flags) as numpy; the flag word starts as garbage."""
    L = tfg._lib
    lib = L.require_gpu()
    n_rows, F = x.shape
    sp = torch.from_numpy(np.asarray(seg_ptr, np.int32)).to(DEV)
    sn = None if seg_node is None else torch.from_numpy(np.asarray(seg_node, np.int32)).to(DEV)
    N = n_rows if sn is None else int(sn.shape[0])
    out = torch.full((G * k, F), 5.0, device=DEV)
    slot_node = torch.full((G * k,), 77, dtype=torch.int32, device=DEV)
    node_slot = torch.full((n_rows,), 77, dtype=torch.int32, device=DEV)
    flags = torch.full((1,), 1 << 20, dtype=torch.int32, device=DEV)
    ldx = x.stride(0) if n_rows > 1 else max(F, 1)
    key = None if sort_col is None else ctypes.c_void_p(x.data_ptr() + 4 * sort_col)
    L.check(lib.tfgx_segment_rows_3d_f32(L.ptr(sp), L.ptr(sn), G, N, L.ptr(x), ldx, n_rows, F, k, key, ldx, L.ptr(out), max(F, 1),
                                         L.ptr(slot_node), L.ptr(node_slot), L.ptr(flags), L.stream_ptr()), "rows3d")
    return out.cpu().numpy(), slot_node.cpu().numpy(), node_slot.cpu().numpy(), int(flags.item())


def _composed(tfg, x, ei, gid, k, si, G):
    px, _, _, pgi = tfg.nn.sort_pool(x, ei, None, gid, k=k, sort_index=si)
    return tfg.utils.convert_x_to_3d(px, pgi, k=k, num_sources=G)


# ---- 1. kernel == mirror == composed route ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, interleave", [(n, False) for n in sorted(BATCHES)] + [(n, True) for n in sorted(BATCHES) if len(BATCHES[n]) > 1],
                         ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else ("interleaved" if v else "in_order"))
def test_kernel_equals_the_mirror_and_the_composed_route(tfg, name, interleave):
    sizes = BATCHES[name]
    G = len(sizes)
    for i, (k, F) in enumerate(COMBOS):
        what = "{} / k={} / F={}".format(name, k, F)
        x_np, gid_np, ei_np = _batch(sizes, F, seed=i, interleave=interleave)
        si = (-1, 0, F // 2)[i % 3]
        x = _dev(x_np, offset=i % 2, pad=(i % 2) * 2)          # odd combos: a column block, base not 16-byte aligned, ldx = F + 3
        gid, ei = torch.from_numpy(gid_np).to(DEV), torch.from_numpy(ei_np).to(DEV)
        seg_ptr, seg_node = graph_plan(gid_np, G)
        # sort mode: the Python surface, the entry point, the mirror and the composed route
        m_out, m_slot, m_node, m_flags = mirror_sort_pool_3d(x_np, gid_np, k, sort_index=si, num_graphs=G, with_index=True)
        assert m_flags == 0
        assert tfg.nn.sort_pool_3d_route(gid, num_graphs=G) == "fused"
        out, slot = tfg.nn.sort_pool_3d(x, gid, k, sort_index=si, num_graphs=G, return_index=True)
        _eq(out, m_out, what + ": sort_pool_3d")
        _eq(slot, m_slot.reshape(G, k), what + ": slot_node")
        r_out, r_slot, r_node, r_flags = _raw(tfg, x, seg_ptr, seg_node, G, k, sort_col=si % F)
        _eq(r_out.reshape(G, k, F), m_out, what + ": entry point")
        _eq(r_slot, m_slot, what + ": entry point slot_node")
        _eq(r_node, m_node, what + ": node_slot")
        assert r_flags == 0, what
        if x_np.shape[0]:
            _eq(_composed(tfg, x, ei, gid, k, si, G), m_out, what + ": composed route")
        # plain mode
        p_out, p_slot, p_node = mirror_convert_x_to_3d(x_np, gid_np, k=k, num_sources=G, with_index=True)
        _eq(tfg.utils.convert_x_to_3d(x, gid, k=k, num_sources=G), p_out, what + ": convert_x_to_3d")
        r_out, r_slot, r_node, r_flags = _raw(tfg, x, seg_ptr, seg_node, G, k)
        _eq(r_out.reshape(G, k, F), p_out, what + ": plain entry point")
        _eq(r_slot, p_slot, what + ": plain slot_node")
        _eq(r_node, p_node, what + ": plain node_slot")
        assert r_flags == 0, what


def test_layer_and_numpy_forms(tfg):
    x_np, gid_np, ei_np = _batch([5, 0, 9, 2], 6, seed=4, interleave=True)
    ref = mirror_sort_pool_3d(x_np, gid_np, 4, sort_index=2)
    layer = tfg.layers.SortPool(k=4, sort_index=2)
    x, gid, ei = (torch.from_numpy(a).to(DEV) for a in (x_np, gid_np, ei_np))
    _eq(layer.pool_3d([x, gid]), ref, "pool_3d of [x, node_graph_index]")
    _eq(layer.pool_3d([x, ei, None, gid], num_graphs=4), ref, "pool_3d of the 4-list")
    got = tfg.nn.sort_pool_3d(x_np, gid_np, 4, sort_index=2)                # numpy in -> numpy out, num_graphs read back
    assert isinstance(got, np.ndarray)
    _eq(got, ref, "numpy in")
    got = tfg.utils.convert_x_to_3d(x_np, gid_np)
    assert isinstance(got, np.ndarray)
    _eq(got, mirror_convert_x_to_3d(x_np, gid_np), "convert_x_to_3d, numpy in")
    cache = {}
    a = tfg.utils.convert_x_to_3d(x, gid, k=3, num_sources=4, cache=cache)
    assert len(cache) == 1
    _eq(tfg.utils.convert_x_to_3d(x, gid, k=3, num_sources=4, cache=cache), a.cpu().numpy(), "warm cache")
    for kw, word in ((dict(k=None), "k must be an integer of at least 1"), (dict(k=0), "at least 1"), (dict(k=2.0), "at least 1"),
                     (dict(k=3, ratio=0.5), "ratio= has no 3-D form"), (dict(k=3, sort_index=6), "sort_index = 6 is no column")):
        with pytest.raises(ValueError, match=word):
            tfg.nn.sort_pool_3d(x, gid, **kw)
    with pytest.raises(ValueError, match="ratio= has no 3-D form"):
        tfg.layers.SortPool(ratio=0.5).pool_3d([x, gid])
    with pytest.raises(ValueError, match="x has 16 rows, the index has 15 entries"):
        tfg.nn.sort_pool_3d(x, gid[:15], 3)


# ---- 2. the reference's recorded outputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_product_equals_the_reference_golden(tfg, case):
    golden = dict(np.load(GOLDEN))
    g = case.inputs()
    n_ref = int(g["gid"].max()) + 1
    for name, k, pad, si in case.configs:
        for num in sc.NUM_SOURCES[case.name]:
            ref = golden["{}::{}/convert".format(case.name, name)]
            got = tfg.utils.convert_x_to_3d(g["x"], g["gid"], k=k, pad=pad, num_sources=num)
            assert got.shape == ((num or n_ref),) + ref.shape[1:], name
            _eq(got[:n_ref], ref, name + ": convert_x_to_3d")
            assert not got[n_ref:].any()
            if k is not None and pad:
                ref = golden["{}::{}/sort".format(case.name, name)]
                got = tfg.nn.sort_pool_3d(g["x"], g["gid"], k, sort_index=si, num_graphs=num)
                _eq(got[:n_ref], ref, name + ": sort_pool_3d")
                assert not got[n_ref:].any()


# ---- 3. ties, zeros and non-finite keys: the selection is topk_pool's ------------------------------------------------------------------
def _key_columns(rng, n):
    runs = np.repeat(rng.standard_normal(n // 5 + 1).astype(np.float32), 5)[:n]
    zeros = rng.choice(np.asarray([-0.0, 0.0, 0.5, -0.5], np.float32), n)
    nonfinite = rng.standard_normal(n).astype(np.float32)
    nonfinite[rng.permutation(n)[:n // 4]] = rng.choice(np.asarray([np.nan, -np.nan, np.inf, -np.inf], np.float32), n // 4)
    return {"all equal": np.full(n, 0.25, np.float32), "tied in runs": runs, "signed zeros": zeros, "NaN and inf": nonfinite}


@pytest.mark.parametrize("k", [1, 30, 5000])
def test_selection_equals_topk_pool_on_ties_zeros_and_non_finite_keys(tfg, k):
    sizes = [0, 3, 64, 0, 257, 2, 1023, 63, MAX_GRAPH_NODES]
    G, F = len(sizes), 4
    x_np, gid_np, ei_np = _batch(sizes, F, seed=9, interleave=True, distinct=False)
    rng = np.random.Generator(np.random.PCG64(10))
    for kind, col in _key_columns(rng, x_np.shape[0]).items():
        x_np[:, 1] = col
        x, gid, ei = (torch.from_numpy(a).to(DEV) for a in (x_np, gid_np, ei_np))
        out, slot = tfg.nn.sort_pool_3d(x, gid, k, sort_index=1, num_graphs=G, return_index=True)
        picked = tfg.nn.topk_pool(gid, x[:, 1], k=k, num_segments=G)
        assert torch.equal(slot.reshape(-1)[slot.reshape(-1) >= 0], picked), kind
        m_out, m_slot, _, _ = mirror_sort_pool_3d(x_np, gid_np, k, sort_index=1, num_graphs=G, with_index=True)
        _eq(slot, m_slot.reshape(G, k), kind + ": mirror slot_node")
        _eq(out, m_out, kind + ": mirror")
        _eq(_composed(tfg, x, ei, gid, k, 1, G), m_out, kind + ": composed route")


# ---- 4. a graph above the LDS cap ----------------------------------------------------------------------------------------------------------
def test_a_graph_above_the_cap_takes_the_composed_route_and_the_kernel_flags_it(tfg):
    sizes, F, k = [5, MAX_GRAPH_NODES + 1, 0, 70], 5, 30
    G = len(sizes)
    x_np, gid_np, ei_np = _batch(sizes, F, seed=11, interleave=True)
    x, gid, ei = (torch.from_numpy(a).to(DEV) for a in (x_np, gid_np, ei_np))
    cache = {}
    assert tfg.nn.sort_pool_3d_route(gid, num_graphs=G, cache=cache) == "composed"
    ref, ref_slot, _, _ = mirror_sort_pool_3d(x_np, gid_np, k, num_graphs=G, with_index=True, cap=1 << 30)
    out, slot = tfg.nn.sort_pool_3d(x, gid, k, num_graphs=G, cache=cache, return_index=True)
    _eq(out, ref, "sort_pool_3d above the cap")
    _eq(slot, ref_slot.reshape(G, k), "slot_node above the cap")
    _eq(_composed(tfg, x, ei, gid, k, -1, G), ref, "the composed route")
    xg = x.clone().requires_grad_(True)
    d = torch.randn(G, k, F, device=DEV)
    tfg.nn.sort_pool_3d(xg, gid, k, num_graphs=G, cache=cache).backward(d)
    node_slot = np.full(x_np.shape[0], -1, np.int32)
    live = ref_slot >= 0
    node_slot[ref_slot[live]] = np.flatnonzero(live)
    _eq(xg.grad, mirror_backward(d.cpu().numpy(), node_slot), "dx above the cap")
    # at the ABI level the long graph is an ordinary flagged input: zero rows, -1 everywhere, the other graphs as ever
    seg_ptr, seg_node = graph_plan(gid_np, G)
    m_out, m_slot, m_node, m_flags = mirror_rows_3d(x_np, seg_ptr, seg_node, G, k, sort_col=F - 1)
    assert m_flags == TOO_LONG and not m_out[k:2 * k].any() and (m_slot[k:2 * k] == -1).all() and (m_node[gid_np == 1] == -1).all()
    r_out, r_slot, r_node, r_flags = _raw(tfg, x, seg_ptr, seg_node, G, k, sort_col=F - 1)
    assert r_flags == TOO_LONG
    _eq(r_out, m_out, "flagged: out")
    _eq(r_slot, m_slot, "flagged: slot_node")
    _eq(r_node, m_node, "flagged: node_slot")
    # the plain mode has no cap
    _eq(tfg.utils.convert_x_to_3d(x, gid, k=MAX_GRAPH_NODES + 1, num_sources=G), mirror_convert_x_to_3d(x_np, gid_np, num_sources=G),
        "convert_x_to_3d of a long graph")


# ---- 5. the backward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, F", [(1, 5), (30, 128), (30, 97), (5000, 4)])
def test_backward_equals_the_composed_route_and_is_reproducible(tfg, k, F):
    sizes = [0, 3, 64, 0, 257, 2, 1023, 63, 0]
    G = len(sizes)
    x_np, gid_np, ei_np = _batch(sizes, F, seed=k, interleave=True)
    gid, ei = torch.from_numpy(gid_np).to(DEV), torch.from_numpy(ei_np).to(DEV)
    d = torch.randn(G, k, F, device=DEV)
    grads = []
    for route in ("fused", "fused", "composed", "plain"):
        x = _dev(x_np, offset=1, pad=2).detach().requires_grad_(True)
        if route == "fused":
            out = tfg.nn.sort_pool_3d(x, gid, k, num_graphs=G)
        elif route == "composed":
            out = _composed(tfg, x, ei, gid, k, -1, G)
        else:
            out = tfg.utils.convert_x_to_3d(x, gid, k=k, num_sources=G)
        out.backward(d)
        grads.append(x.grad.cpu().numpy())
    _, _, node_slot, _ = mirror_sort_pool_3d(x_np, gid_np, k, num_graphs=G, with_index=True)
    ref = mirror_backward(d.cpu().numpy(), node_slot)
    _eq(grads[0], ref, "dx: mirror")
    _eq(grads[1], grads[0], "dx: the second run")
    _eq(grads[2], grads[0], "dx: composed route")
    assert not grads[0][node_slot < 0].any()                     # the rows of nodes cut off by k are exactly zero
    if k < 1023:
        assert (node_slot < 0).any()
    _eq(grads[3], mirror_backward(d.cpu().numpy(), mirror_convert_x_to_3d(x_np, gid_np, k=k, num_sources=G, with_index=True)[2]),
        "dx: convert_x_to_3d")


# ---- 6. static batches -------------------------------------------------------------------------------------------------------------------
SIZES = [(0, 0), (1, 1), (2, 3), (3, 5), (7, 12), (33, 70), (64, 130), (65, 140), (256, 500), (257, 520), (6, 0), (1025, 2000)]
STATIC_BATCHES = {"dead first, in the middle and last, a graph twice": [-1, 7, 0, -1, 8, 9, 3, 3, -1],
                  "all dead": [-1, -1, -1, -1],
                  "every size": [5, 6, 11, 9, 8, 7, 4, 10, 1, 2]}
SF = 6
_WORLD = {}


def _store():
    if "s" not in _WORLD:
        import tf_geometric_amd as tfg
        d = random_dataset(np.random.Generator(np.random.PCG64(31)), SIZES, SF, y=False)
        d["y"] = (np.arange(len(SIZES), dtype=np.int64) % 3).reshape(-1, 1)
        _WORLD["s"] = tfg.data.GraphStore.from_arrays(**d)
    return _WORLD["s"]


def _ids(ids):
    return torch.tensor(ids, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("name", sorted(STATIC_BATCHES), ids=lambda v: v.replace(" ", "_"))
def test_static_forms_equal_sort_pool_3d_on_the_live_graphs(tfg, name):
    store = _store()
    ids = STATIC_BATCHES[name]
    B = len(ids)
    live = [i for i in ids if i >= 0]
    live_slots = [j for j, i in enumerate(ids) if i >= 0]
    batch = store.collate_static(_ids(ids))
    plain = store.collate(live) if live else None
    h = torch.randn(batch.capacities.n_cap, SF, device=DEV)      # the padded rows hold values too: they are never read
    n_live = int(batch.counts[1])
    if plain is not None:
        h[:n_live] = plain.x
    layer = tfg.layers.SortPool(k=30, sort_index=1)
    for k, si in ((1, -1), (30, 1), (300, 0)):
        out, slot = tfg.nn.sort_pool_static(h, batch, k, sort_index=si, return_index=True)
        assert tuple(out.shape) == (B, k, SF) and tuple(slot.shape) == (B, k)
        dead = [j for j in range(B) if j not in live_slots]
        assert not out[dead].any() and bool((slot[dead] == -1).all()), "dead slots are exactly zero"
        if plain is not None:
            ref, ref_slot = tfg.nn.sort_pool_3d(plain.x, plain.node_graph_index, k, sort_index=si, num_graphs=len(live),
                                                cache=plain.cache, return_index=True)
            assert torch.equal(out[live_slots], ref) and torch.equal(slot[live_slots], ref_slot), (name, k)
            assert torch.equal(batch.to_3d(h, k)[live_slots],
                               tfg.utils.convert_x_to_3d(plain.x, plain.node_graph_index, k=k, num_sources=len(live), cache=plain.cache))
        assert not batch.to_3d(h, k)[dead].any()
        m_out = mirror_sort_pool_3d(h[:n_live].cpu().numpy(), batch.node_graph_index[:n_live].cpu().numpy(), k, sort_index=si,
                                    num_graphs=B) if n_live else np.zeros((B, k, SF), np.float32)
        _eq(out, m_out, "{} k={}: mirror".format(name, k))
    assert torch.equal(layer.pool_static(h, batch), tfg.nn.sort_pool_static(h, batch, 30, sort_index=1))
    assert int(batch.counts[3]) == 0 and batch.check() is batch
    # after one SAGPool level: the pooled batch's own rows and row offsets
    score = torch.randn(batch.capacities.n_cap, device=DEV)
    pooled = tfg.nn.sag_pool_static(h, batch, lambda inputs, training=None, cache=None: score, ratio=0.5)
    m_live = int(pooled.counts[1])
    for k in (2, 30):
        out = tfg.nn.sort_pool_static(pooled.x, pooled, k, sort_index=2)
        m_out = mirror_sort_pool_3d(pooled.x[:m_live].detach().cpu().numpy(), pooled.node_graph_index[:m_live].cpu().numpy(), k,
                                    sort_index=2, num_graphs=B) if m_live else np.zeros((B, k, SF), np.float32)
        _eq(out, m_out, "{} k={}: after one level".format(name, k))
        _eq(pooled.to_3d(pooled.x, k), mirror_convert_x_to_3d(pooled.x[:m_live].detach().cpu().numpy(),
                                                               pooled.node_graph_index[:m_live].cpu().numpy(), k=k, num_sources=B)
            if m_live else np.zeros((B, k, SF), np.float32), "{} k={}: to_3d after one level".format(name, k))
    assert pooled.check() is pooled


def test_static_backward_reaches_the_live_rows_only(tfg):
    store = _store()
    batch = store.collate_static(_ids([-1, 7, 0, -1, 8, 9, 3, 3, -1]))
    n_cap, n_live = batch.capacities.n_cap, int(batch.counts[1])
    h = torch.randn(n_cap, SF, device=DEV, requires_grad=True)
    out, slot = tfg.nn.sort_pool_static(h, batch, 4, return_index=True)
    d = torch.randn_like(out)
    out.backward(d)
    slot = slot.reshape(-1).cpu().numpy()
    node_slot = np.full(n_cap, -1, np.int32)
    node_slot[slot[slot >= 0]] = np.flatnonzero(slot >= 0)
    _eq(h.grad, mirror_backward(d.cpu().numpy(), node_slot), "static dx")
    assert not h.grad[n_live:].any()


def test_static_refusals_name_their_argument(tfg):
    store = _store()
    batch = store.collate_static(_ids([5, 6, -1, 4]))
    n_cap = batch.capacities.n_cap
    plain = store.collate([5, 6])
    h = torch.zeros(n_cap, SF, device=DEV)
    with pytest.raises(ValueError, match="sort_pool_static: batch must be a StaticBatchGraph"):
        tfg.nn.sort_pool_static(plain.x, plain, 3)
    with pytest.raises(ValueError, match="sort_pool_static: batch must be a StaticBatchGraph"):
        tfg.layers.SortPool(k=3).pool_static(plain.x, plain)
    with pytest.raises(ValueError, match=r"sort_pool_static: x must have one row per row of the batch \(\[{}, F\]\)".format(n_cap)):
        tfg.nn.sort_pool_static(h[:-1], batch, 3)
    with pytest.raises(ValueError, match=r"StaticBatchGraph.to_3d: x must have one row per row of the batch"):
        batch.to_3d(h[:-1], 3)
    with pytest.raises(ValueError, match="sort_pool_static: k must be an integer of at least 1"):
        tfg.nn.sort_pool_static(h, batch, 0)
    with pytest.raises(ValueError, match="ratio= has no 3-D form"):
        tfg.layers.SortPool(ratio=0.5).pool_static(h, batch)
    big = random_dataset(np.random.Generator(np.random.PCG64(1)), [(3, 2), (MAX_GRAPH_NODES + 1, 4)], SF)
    long_store = tfg.data.GraphStore.from_arrays(**big)
    long_batch = long_store.collate_static(_ids([0, -1]))
    with pytest.raises(ValueError, match="sort_pool_static: the store's largest graph has {} nodes, more than the {}".format(
            MAX_GRAPH_NODES + 1, MAX_GRAPH_NODES)):
        tfg.nn.sort_pool_static(torch.zeros(long_batch.capacities.n_cap, SF, device=DEV), long_batch, 3)
    # the flag word is ORed into counts[3] on the device, and check() names it
    batch.counts[3:4].bitwise_or_(torch.tensor([TOO_LONG], dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="more than {} nodes".format(MAX_GRAPH_NODES)):
        batch.check()


# ---- 7. no host read ---------------------------------------------------------------------------------------------------------------------
def test_static_and_warm_cache_forms_make_no_host_read(tfg, monkeypatch):
    from tf_geometric_amd.plan import CsrPlan
    store = _store()
    ids = _ids([5, -1, 6, 9, 4])
    cap = store.static_capacities(5)
    plain = store.collate([5, 6, 9, 4])
    w = torch.randn(SF, SF, device=DEV, requires_grad=True)

    def run():
        w.grad = None
        batch = store.collate_static(ids, cap)
        h = batch.x @ w
        loss = tfg.nn.sort_pool_static(h, batch, 30).sum() + batch.to_3d(h, 7).sum()
        hp = plain.x @ w
        loss = loss + tfg.nn.sort_pool_3d(hp, plain.node_graph_index, 30, num_graphs=4, cache=plain.cache).sum()
        loss = loss + tfg.utils.convert_x_to_3d(hp, plain.node_graph_index, k=7, num_sources=4, cache=plain.cache).sum()
        loss.backward()
        return loss

    run()                                                       # the warm call

    def no_build(*a, **k):
        raise AssertionError("a plan was built by sorting")

    monkeypatch.setattr(CsrPlan, "build", staticmethod(no_build))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss) and torch.isfinite(w.grad).all() and bool(w.grad.any())


# ---- 8. capture ---------------------------------------------------------------------------------------------------------------------------
def test_sort_pool_still_refuses_a_capture(tfg, monkeypatch):
    x_np, gid_np, ei_np = _batch([5, 9], 4, seed=2, interleave=False)
    x, gid, ei = (torch.from_numpy(a).to(DEV) for a in (x_np, gid_np, ei_np))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="sort_pool cannot run inside a hipGraph capture"):
        tfg.nn.sort_pool(x, ei, None, gid, k=3)


def test_example_step_replayed_equals_eager_with_dropout_on(tfg):
    """examples/demo_sort_pool.py through demo_sag_pool_h.make_static_step: with the model's dropout 0.5 ON, four replays of the
    captured step (ids -> collate_static -> 3 x GCN -> SortPool.pool_static -> Conv1D -> MLP -> loss -> backward -> Adam) give
    the losses of four eager static steps from the same weights, within 1e-6 of |loss|."""
    import demo_sort_pool as demo
    data = demo.make_dataset(48, 3)
    store = demo.graph_store(data, range(48))
    cap = store.static_capacities(16)
    losses = {}
    for capture in (False, True):
        torch.manual_seed(5)
        model = demo.SortPoolModel(data.num_features, data.num_classes, seed=5, fused=True)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
        loader = store.static_loader(16, shuffle=True, seed=6)
        step = demo.make_static_step(model, store, loader, cap, opt, capture, loss=demo.static_loss)
        losses[capture] = [float(step().detach()) for _ in range(4)]
        assert int(loader.cursor) == 64
    print("eager    ", losses[False])
    print("replayed ", losses[True], " bit-equal:", losses[True] == losses[False])
    assert len(set(losses[False])) == 4
    for c, e in zip(losses[True], losses[False]):
        assert abs(c - e) <= 1e-6 * abs(e), losses


def test_example_routes_agree(tfg):
    """The example's three readouts — SortPool + convert_x_to_3d, SortPool.pool_3d, SortPool.pool_static — give the same logits
    for the same graphs (dropout off)."""
    import demo_sort_pool as demo
    data = demo.make_dataset(24, 1)
    model = demo.SortPoolModel(data.num_features, data.num_classes, seed=2)
    x, ei, gid, y, G = demo.make_batch(data, list(range(12)))
    with torch.no_grad():
        composed = model([x, ei, gid, G])
        model.fused = True
        fused = model([x, ei, gid, G])
        store = demo.graph_store(data, range(12))
        static = demo.static_logits(model, store.collate_static(_ids(list(range(12)))))
    assert torch.equal(composed, fused)
    assert float((static - fused).abs().max()) <= 1e-5 * float(fused.abs().max())      # other GCN launch shapes (padded rows)


# ---- 9. model level: float64 autograd -------------------------------------------------------------------------------------------------------
def test_two_gcn_sort_pool_dense_model_equals_float64(tfg):
    """2 x GCN(relu) -> sort_pool_3d(k) -> dense on the flattened [G, k * F]: logits and every parameter gradient against float64
    autograd; the float64 side takes the device's slot_node (it does not re-decide near-ties).  Each entry within 1e-5 of the
    tensor's largest reference magnitude."""
    from tf_geometric_amd import autograd as AG
    sizes, F_in, U, k, C = [7, 0, 33, 12, 64, 3], 5, 8, 10, 3
    G = len(sizes)
    x_np, gid_np, _ = _batch(sizes, F_in, seed=21, interleave=True)
    rng = np.random.Generator(np.random.PCG64(22))
    n = x_np.shape[0]
    ei_np = np.concatenate([rng.choice(np.flatnonzero(gid_np == g), (2, 3 * s)) for g, s in enumerate(sizes) if s], axis=1).astype(np.int32)
    y = torch.from_numpy(rng.integers(0, C, G)).to(DEV)
    x, gid, ei = (torch.from_numpy(a).to(DEV) for a in (x_np, gid_np, ei_np))
    gcns = [tfg.layers.GCN(U, activation=tfg.relu, seed=3 + i) for i in range(2)]
    for i, g in enumerate(gcns):
        g._maybe_build([torch.empty(1, F_in if i == 0 else U)])
        g.trainable(True)
    gen = torch.Generator(device="cpu").manual_seed(5)
    dense_k = ((torch.rand((k * U, C), generator=gen) - 0.5) * 0.5).to(DEV).requires_grad_(True)
    dense_b = torch.linspace(-0.2, 0.3, C, device=DEV).requires_grad_(True)
    params = gcns[0].parameters() + gcns[1].parameters() + [dense_k, dense_b]
    with torch.no_grad():
        for p in params[:4]:
            if p.dim() == 1:
                p.copy_(torch.linspace(-0.2, 0.3, p.numel(), device=DEV))
    h = x
    for g in gcns:
        h = g([h, ei, None], training=True)
    h3, slot = tfg.nn.sort_pool_3d(h, gid, k, num_graphs=G, return_index=True)
    logits = AG.linear(h3.reshape(G, k * U), dense_k, dense_b)
    torch.nn.functional.cross_entropy(logits, y).backward()

    leaves = [p.detach().cpu().double().requires_grad_(True) for p in params]
    row, col = torch.from_numpy(ei_np[0].astype(np.int64)), torch.from_numpy(ei_np[1].astype(np.int64))

    def gcn64(hh, kk, bias):
        dis = (torch.zeros(n, dtype=torch.float64).index_add_(0, row, torch.ones(row.shape[0], dtype=torch.float64)) + 1.0).pow(-0.5)
        hk = hh @ kk
        pre = torch.zeros_like(hk).index_add_(0, row, (dis[row] * dis[col])[:, None] * hk[col]) + (dis * dis)[:, None] * hk + bias
        return torch.relu(pre)

    h64 = gcn64(gcn64(torch.from_numpy(x_np).double(), leaves[0], leaves[1]), leaves[2], leaves[3])
    s = torch.from_numpy(slot.reshape(-1).cpu().numpy().astype(np.int64))
    rows = torch.where((s >= 0)[:, None], h64[s.clamp(min=0)], torch.zeros((), dtype=torch.float64))
    logits64 = rows.reshape(G, k * U) @ leaves[4] + leaves[5]
    torch.nn.functional.cross_entropy(logits64, y.cpu()).backward()
    for what, got, ref in [("logits", logits, logits64)] + [("d/d parameter {}".format(i), p.grad, q.grad)
                                                           for i, (p, q) in enumerate(zip(params, leaves))]:
        got, ref = got.detach().cpu().double().numpy(), ref.detach().numpy()
        err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
        print("{}: max|difference| = {:.3e}, largest reference magnitude = {:.3e}".format(what, err, scale))
        assert err <= 1e-5 * scale, what
