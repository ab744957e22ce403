# coding=utf-8
"""include/tfgx_collate_static.h (fixed-shape batches) without a GPU: the numpy mirror of the whole operator, whose plans are put
together the way the kernel does it (the live part of mirror_collate, closed-form dead rows, an identity tail) and shown to BE
the stable sorts of its own padded lists; the capacity arithmetic of GraphStore.static_capacities; every argument refusal and
every zero-size success of both entry points.  (The header / table / version / struct checks are tests/test_abi_registry.py's.)"""
import ctypes

import numpy as np
import pytest

from test_collate_abi import mirror_collate, random_dataset
from test_drop_edge_abi import mirror_plan

BAD_ID, OVERFLOW = 1, 2


# ---- the mirror: test infrastructure shared with the GPU tests ----------------------------------------------------------
def mirror_capacities(node_ptr, edge_ptr, B, max_nodes=None, max_edges=None, sink_degree=32):
    """(max_nodes, max_edges, P, n_cap, e_cap) by the arithmetic the header states."""
    if max_nodes is None:
        max_nodes = int(np.sort(np.diff(node_ptr))[::-1][:B].sum())
    if max_edges is None:
        max_edges = int(np.sort(np.diff(edge_ptr))[::-1][:B].sum())
    P = max(1, -(-max_edges // sink_degree))
    return max_nodes, max_edges, P, max_nodes + P, max_edges


def mirror_live(node_ptr, edge_ptr, ids, max_nodes, max_edges):
    """(live mask [B], flags): in range, and both totals cumulated over the in-range slots through the slot within the bounds."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    G = len(node_ptr) - 1
    in_range = (ids >= 0) & (ids < G)
    safe = np.where(in_range, ids, 0)
    cn = np.cumsum(np.where(in_range, node_ptr[safe + 1] - node_ptr[safe], 0))
    ce = np.cumsum(np.where(in_range, edge_ptr[safe + 1] - edge_ptr[safe], 0))
    live = in_range & (cn <= max_nodes) & (ce <= max_edges)
    flags = (BAD_ID if ((ids < -1) | (ids >= G)).any() else 0) | (OVERFLOW if (in_range & ~live).any() else 0)
    return live, flags


def mirror_collate_static(x, edge_index, edge_weight, node_ptr, edge_ptr, ids, max_nodes=None, max_edges=None, sink_degree=32):
    """numpy restatement of GraphStore.collate_static: a dict with the padded x, edge_index, edge_weight, node_graph_index,
    edge_graph_index, graph_mask, counts, and plan / plan_t / graph_plan as (row_ptr, col, perm), ASSEMBLED (not sorted): the live
    part is mirror_collate's, a dead row's offset is e_live plus the padded edges of the sinks before it, the tail is the
    identity."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    B = len(ids)
    max_nodes, max_edges, P, n_cap, e_cap = mirror_capacities(node_ptr, edge_ptr, B, max_nodes, max_edges, sink_degree)
    live, flags = mirror_live(node_ptr, edge_ptr, ids, max_nodes, max_edges)
    slots = np.nonzero(live)[0].astype(np.int32)
    m = mirror_collate(x, edge_index, edge_weight, node_ptr, edge_ptr, ids[live])
    n_live, e_live = m["x"].shape[0], m["edge_index"].shape[1]
    assert n_live <= max_nodes and e_live <= max_edges
    F = x.shape[1]
    tail = np.arange(e_cap - e_live)
    sink_of = (n_cap - P + tail // sink_degree).astype(np.int32)
    assert e_live == e_cap or sink_of.max() < n_cap
    out = {"x": np.concatenate([m["x"], np.zeros((n_cap - n_live, F), np.float32)]),
           "edge_index": np.concatenate([m["edge_index"], np.stack([sink_of, sink_of])], axis=1).astype(np.int32),
           "edge_weight": np.concatenate([m["edge_weight"], np.ones(e_cap - e_live, np.float32)]),
           "node_graph_index": np.concatenate([slots[m["node_graph_index"]], np.full(n_cap - n_live, B, np.int32)]).astype(np.int32),
           "edge_graph_index": np.concatenate([slots[m["edge_graph_index"]], np.full(e_cap - e_live, B, np.int32)]).astype(np.int32),
           "graph_mask": live, "counts": np.asarray([live.sum(), n_live, e_live, flags], dtype=np.int32),
           "live_ids": ids[live], "n_live": n_live, "e_live": e_live, "sinks": P, "n_cap": n_cap, "e_cap": e_cap}
    dead_rows = np.arange(n_live, n_cap + 1)
    dead_ptr = e_live + np.minimum(e_cap - e_live, np.maximum(dead_rows - (n_cap - P), 0) * sink_degree)
    for key in ("plan", "plan_t"):
        row_ptr, col, perm = m[key]
        out[key] = (np.concatenate([row_ptr[:n_live], dead_ptr]).astype(np.int32), np.concatenate([col, sink_of]).astype(np.int32),
                    np.concatenate([perm, e_live + tail]).astype(np.int32))
    sizes = np.where(live, node_ptr[np.where(live, ids, 0) + 1] - node_ptr[np.where(live, ids, 0)], 0)
    nodes = np.arange(n_cap, dtype=np.int32)
    out["graph_plan"] = (np.concatenate([[0], np.cumsum(sizes), [n_cap]]).astype(np.int32), nodes, nodes)
    return out


SIZES = [(3, 4), (0, 0), (5, 0), (2, 6), (1, 1), (0, 0), (7, 20), (40, 100)]
G = len(SIZES)
BATCHES = {"all live": [0, 1, 2, 3, 4, 5, 6, 7], "dead first": [-1, 3, 6], "dead in the middle": [3, -1, -1, 6], "dead last": [6, 3, -1],
           "only dead": [-1, -1, -1], "a graph three times": [6, 6, 6], "empty graphs": [1, 5, 1], "no slot": [],
           "bad ids": [3, G, 6, G + 7, -2, 0], "one": [7]}


def _dataset(F=5, seed=1):
    return random_dataset(np.random.Generator(np.random.PCG64(seed)), SIZES, F)


def _args(d):
    return d["x"], d["edge_index"], d["edge_weight"], d["node_ptr"], d["edge_ptr"]


@pytest.mark.parametrize("sink_degree", [1, 3, 32])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_mirror_plans_are_the_stable_sorts_of_its_padded_lists(name, sink_degree):
    """The identity-tail claim: the assembled plans equal a stable sort of the padded list, of its flip and of the graph index."""
    d = _dataset()
    ids = BATCHES[name]
    for bounds in ({}, {"max_nodes": 12, "max_edges": 30}, {"max_nodes": 50, "max_edges": 7}, {"max_nodes": 0, "max_edges": 0}):
        m = mirror_collate_static(*_args(d), ids, sink_degree=sink_degree, **bounds)
        n_cap, e_cap, B = m["n_cap"], m["e_cap"], len(ids)
        assert m["x"].shape == (n_cap, 5) and m["edge_index"].shape == (2, e_cap) and m["edge_weight"].shape == (e_cap,)
        for key, ei in (("plan", m["edge_index"]), ("plan_t", m["edge_index"][[1, 0]])):
            for got, ref, part in zip(m[key], mirror_plan(ei, n_cap), ("row_ptr", "col", "perm")):
                assert np.array_equal(got, ref) and got.dtype == ref.dtype, (name, bounds, key, part)
        ref = mirror_plan(np.stack([m["node_graph_index"], np.arange(n_cap, dtype=np.int32)]), B + 1)
        for got, r, part in zip(m["graph_plan"], ref, ("row_ptr", "col", "perm")):
            assert np.array_equal(got, r), (name, bounds, "graph_plan", part)
        # the padding is inert: dead rows are zero and belong to graph B, no edge joins a live row and a dead one, and no sink
        # has more than sink_degree edges
        n_live, e_live, P = m["n_live"], m["e_live"], m["sinks"]
        assert not m["x"][n_live:].any() and (m["node_graph_index"][n_live:] == B).all() and n_live <= n_cap - P
        assert (m["edge_index"][:, :e_live] < n_live).all() and (m["edge_index"][:, e_live:] >= n_cap - P).all()
        assert (m["edge_index"][0, e_live:] == m["edge_index"][1, e_live:]).all() and (m["edge_weight"][e_live:] == 1.0).all()
        assert np.bincount(m["edge_index"][0, e_live:], minlength=n_cap).max(initial=0) <= sink_degree
        assert m["counts"][0] == m["graph_mask"].sum() and (m["counts"][3] & BAD_ID != 0) == (name == "bad ids")


def test_mirror_live_part_is_collate_of_the_live_ids_and_overflow_drops_a_suffix():
    d = _dataset()
    ids = [6, 3, -1, 7, 0, 4]                                   # nodes 7, 2, -, 40, 3, 1; edges 20, 6, -, 100, 4, 1
    m = mirror_collate_static(*_args(d), ids)
    assert m["graph_mask"].tolist() == [True, True, False, True, True, True] and m["counts"].tolist() == [5, 53, 131, 0]
    ref = mirror_collate(*_args(d), [6, 3, 7, 0, 4])
    for key in ("x", "edge_index", "edge_weight"):
        assert np.array_equal(m[key][..., :ref[key].shape[-1]] if key == "edge_index" else m[key][:ref[key].shape[0]], ref[key])
    assert m["node_graph_index"][:53].tolist() == [0] * 7 + [1] * 2 + [3] * 40 + [4] * 3 + [5]
    # max_nodes = 9 holds slots 0 and 1 exactly; slot 3 overflows, and the smaller slots after it are dropped with it
    m = mirror_collate_static(*_args(d), ids, max_nodes=9, max_edges=1000)
    assert m["graph_mask"].tolist() == [True, True, False, False, False, False] and m["counts"].tolist() == [2, 9, 26, OVERFLOW]
    m = mirror_collate_static(*_args(d), ids, max_nodes=1000, max_edges=25)
    assert m["graph_mask"].tolist() == [True, False, False, False, False, False] and m["counts"].tolist() == [1, 7, 20, OVERFLOW]


# ---- capacities ---------------------------------------------------------------------------------------------------------
def test_static_capacities_is_the_stated_arithmetic():
    import tf_geometric_amd as tfg
    d = _dataset(3, 2)
    store = tfg.data.GraphStore.from_arrays(**d)
    nodes, edges = sorted((n for n, _ in SIZES), reverse=True), sorted((e for _, e in SIZES), reverse=True)
    for B in (0, 1, 3, G, G + 5):
        cap = store.static_capacities(B)
        assert isinstance(cap, tfg.data.StaticBatchCapacities) and cap.batch_size == B and cap.sink_degree == 32
        assert cap.max_nodes == sum(nodes[:B]) and cap.max_edges == sum(edges[:B]) == cap.e_cap
        assert cap.sinks == max(1, -(-cap.max_edges // 32)) and cap.n_cap == cap.max_nodes + cap.sinks
        assert (cap.max_nodes, cap.max_edges, cap.sinks, cap.n_cap, cap.e_cap) == mirror_capacities(d["node_ptr"], d["edge_ptr"], B)
    # P at max_edges = 0, one below a multiple of sink_degree, at a multiple, one above
    for max_edges, sd, P in ((0, 32, 1), (63, 32, 2), (64, 32, 2), (65, 32, 3), (31, 32, 1), (32, 32, 1), (5, 1, 5), (0, 1, 1)):
        cap = store.static_capacities(4, max_nodes=10, max_edges=max_edges, sink_degree=sd)
        assert (cap.sinks, cap.n_cap, cap.e_cap, cap.max_nodes, cap.sink_degree) == (P, 10 + P, max_edges, 10, sd)
    for kw in (dict(batch_size=-1), dict(batch_size=2.0), dict(batch_size=True), dict(batch_size=2, sink_degree=0),
               dict(batch_size=2, max_nodes=-1), dict(batch_size=2, max_edges=1.5)):
        with pytest.raises(ValueError, match="static_capacities: " + [k for k in kw][-1]):
            store.static_capacities(**kw)
    with pytest.raises(ValueError, match="more than collate_static indexes"):
        store.static_capacities(2, max_nodes=(1 << 31) - 2)
    with pytest.raises(ValueError, match="more than collate_static indexes"):
        store.static_capacities(tfg._lib.COLLATE_STATIC_MAX_SLOTS + 1)


# ---- refusals and zero-size calls -----------------------------------------------------------------------------------------
TABLE_OK = dict(ids=1 << 30, B=8, node_ptr=2 << 30, edge_ptr=3 << 30, G=40, max_nodes=100, max_edges=300, table=4 << 30,
                live_mask=5 << 30, counts=6 << 30, stream=None)


def _table(lib, **kw):
    return lib.tfgx_static_batch_table(*dict(TABLE_OK, **kw).values())


FAKE = dict(ds_x=1 << 30, ds_ldx=8, F=8, ds_row=2 << 30, ds_col=3 << 30, ds_w=4 << 30, ds_n=100, ds_e=300, table=5 << 30, B=4,
            n_cap=54, e_cap=120, sinks=4, sink_degree=32, out_x=6 << 30, out_ldx=8, out_node_graph_index=7 << 30, out_row=8 << 30,
            out_col=9 << 30, out_edge_graph_index=10 << 30, out_w=11 << 30, graph_row_ptr=18 << 30)
FAKE_PLAN = dict(ds_row_ptr=12 << 30, ds_col=13 << 30, ds_perm=14 << 30, out_row_ptr=15 << 30, out_col=16 << 30,
                 out_perm=17 << 30)


def _call(lib, plan=FAKE_PLAN, plan_t=FAKE_PLAN, **kw):
    from tf_geometric_amd import _lib as L
    a = L.CollateStaticArgs(**dict(FAKE, **kw))
    keep = []
    for name, p in (("plan", plan), ("plan_t", plan_t)):
        if p is not None:
            keep.append(L.CollatePlan(**p))
            setattr(a, name, ctypes.pointer(keep[-1]))
    return lib.tfgx_static_batch(ctypes.byref(a), None)


def test_collate_static_names_and_constants():
    from abi_header import declarations, macro
    from tf_geometric_amd import _lib as L
    header = "tfgx_collate_static.h"
    assert sorted(declarations(header)) == sorted(L.COLLATE_STATIC_SIGNATURES) == [
        "tfgx_static_batch", "tfgx_static_batch_table", "tfgx_static_batch_version"]
    assert macro(header, "TFGX_STATIC_BATCH_MAX_SLOTS") == L.COLLATE_STATIC_MAX_SLOTS >= 65535
    assert macro(header, "TFGX_STATIC_BATCH_BAD_ID") == L.COLLATE_STATIC_BAD_ID == BAD_ID
    assert macro(header, "TFGX_STATIC_BATCH_OVERFLOW") == L.COLLATE_STATIC_OVERFLOW == OVERFLOW
    assert macro(header, "TFGX_STATIC_BATCH_DEAD") == L.COLLATE_STATIC_DEAD == -1


def test_collate_static_argument_validation_without_gpu():
    """Every refusal returns TFGX_ERR_INVALID_ARG (1) on the host, before any device work (the pointers are not memory), with
    the entry point and the argument named."""
    from tf_geometric_amd import _lib as L
    lib = L.load_library()

    def refused(rc, entry, word):
        assert rc == 1, rc
        msg = lib.tfgx_last_error()
        assert word in msg and entry + b":" in msg, (word, msg)

    T = b"tfgx_static_batch_table"
    for name in ("B", "G", "max_nodes", "max_edges"):
        refused(_table(lib, **{name: -1}), T, b"negative size (" + name.encode())
        refused(_table(lib, **{name: 1 << 31}), T, name.encode() + b" = 2147483648 does not fit int32")
    refused(_table(lib, B=L.COLLATE_STATIC_MAX_SLOTS + 1), T, b"B = 1048577 is more than the 1048576 slots")
    for name in ("ids", "node_ptr", "edge_ptr", "table", "live_mask", "counts"):
        refused(_table(lib, **{name: None}), T, name.encode() + b" is null")
    refused(_table(lib, B=0, table=None), T, b"table is null")
    refused(_table(lib, B=0, counts=None), T, b"counts is null")

    S = b"tfgx_static_batch"
    refused(lib.tfgx_static_batch(None, None), S, b"args is null")
    for member in ("ds_ldx", "F", "ds_n", "ds_e", "B", "n_cap", "e_cap", "sinks", "sink_degree", "out_ldx"):
        refused(_call(lib, **{member: -1}), S, b"negative size (" + member.encode())
        refused(_call(lib, **{member: 1 << 31}), S, member.encode() + b" = 2147483648 does not fit int32")
    refused(_call(lib, sink_degree=0), S, b"sink_degree = 0 must be at least 1")
    refused(_call(lib, sinks=55), S, b"sinks = 55 is more than n_cap = 54")
    refused(_call(lib, sinks=3), S, b"sinks = 3 of sink_degree = 32 cannot hold a tail of e_cap = 120")
    refused(_call(lib, ds_ldx=7), S, b"ds_ldx = 7 is smaller than F")
    refused(_call(lib, out_ldx=7), S, b"out_ldx = 7 is smaller than F")
    for member in ("table", "graph_row_ptr", "ds_x", "out_x", "out_node_graph_index", "ds_row", "ds_col", "out_row", "out_col",
                   "out_edge_graph_index"):
        refused(_call(lib, **{member: None}), S, member.encode() + b" is null")
    refused(_call(lib, plan=None), S, b"plan is null")
    refused(_call(lib, plan_t=None), S, b"plan_t is null")
    for member in FAKE_PLAN:
        p = dict(FAKE_PLAN, **{member: None})
        refused(_call(lib, plan=p), S, b"plan->" + member.encode() + b" is null")
        refused(_call(lib, plan_t=p), S, b"plan_t->" + member.encode() + b" is null")


def test_collate_static_zero_size_calls_succeed_without_gpu():
    """Where nothing exists to be written nothing is launched: a table of no slots that is not asked for, a batch of no rows and
    no edges with nowhere to put its offsets.  (What an empty batch does write is the GPU tests'.)"""
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    assert _table(lib, B=0, table=None, counts=None) == 0, lib.tfgx_last_error()
    assert _table(lib, B=0, ids=None, node_ptr=None, edge_ptr=None, live_mask=None, table=None, counts=None, G=0, max_nodes=0,
                  max_edges=0) == 0, lib.tfgx_last_error()
    nothing = dict(ds_x=None, ds_row=None, ds_col=None, ds_w=None, table=None, out_x=None, out_node_graph_index=None,
                   out_row=None, out_col=None, out_edge_graph_index=None, out_w=None, graph_row_ptr=None)
    assert _call(lib, plan=None, plan_t=None, n_cap=0, e_cap=0, sinks=0, **nothing) == 0, lib.tfgx_last_error()
    assert _call(lib, plan=None, plan_t=None, n_cap=0, e_cap=0, sinks=0, B=0, ds_n=0, ds_e=0, F=0, ds_ldx=0, out_ldx=0, **nothing) == 0


def test_collate_static_needs_a_gpu_and_refuses_on_the_host_first():
    import torch
    import tf_geometric_amd as tfg
    store = tfg.data.GraphStore.from_arrays(**_dataset(3, 5))
    with pytest.raises(ValueError, match="batch_size"):
        store.static_loader(0)
    if torch.cuda.is_available():
        return
    with pytest.raises(tfg._lib.TfgxError):
        store.collate_static([0, 1])
