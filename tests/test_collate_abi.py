# coding=utf-8
"""include/tfgx_collate.h (minibatch assembly out of a packed device dataset) without a GPU: the exact list of its names, which
no other header's table and not tfgx.h know (the uniform header / table / version / struct checks are
tests/test_abi_registry.py's), the tile the data module uses, every refusal happens on the host with the member named, the zero-size calls succeed; the numpy mirror
of the whole operator (outputs and the three plans; the exact reference of tests/test_gpu_collate.py) keeps its promises; and
the host side of tfg.data.GraphStore — refusals that name the graph, IndexError, the batch table's ptr arithmetic."""
import ctypes

import numpy as np
import pytest

from abi_header import declarations, macro, source
from test_drop_edge_abi import mirror_plan

HEADER = "tfgx_collate.h"


# ---- the mirror: test infrastructure shared with the GPU tests ----------------------------------------------------------
def mirror_collate(x, edge_index, edge_weight, node_ptr, edge_ptr, ids):
    """numpy restatement of GraphStore.collate over the packed arrays (edge_index in dataset-global ids): a dict with
    x, edge_index, edge_weight, node_graph_index, edge_graph_index, and plan / plan_t / graph_plan as (row_ptr, col, perm) of a
    STABLE SORT of the emitted list, of its flip and of (node_graph_index, node id)."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    xs, eis, ws, ngi, egi, off = [], [], [], [], [], 0
    for j, g in enumerate(ids):
        n0, n1, e0, e1 = node_ptr[g], node_ptr[g + 1], edge_ptr[g], edge_ptr[g + 1]
        xs.append(x[n0:n1])
        eis.append(edge_index[:, e0:e1].astype(np.int64) - n0 + off)
        ws.append(edge_weight[e0:e1])
        ngi.append(np.full(n1 - n0, j, np.int32))
        egi.append(np.full(e1 - e0, j, np.int32))
        off += n1 - n0
    F = x.shape[1]
    out = {"x": np.concatenate(xs).reshape(-1, F) if xs else np.zeros((0, F), np.float32),
           "edge_index": (np.concatenate(eis, axis=1) if eis else np.zeros((2, 0))).astype(np.int32),
           "edge_weight": np.concatenate(ws).astype(np.float32) if ws else np.zeros(0, np.float32),
           "node_graph_index": np.concatenate(ngi) if ngi else np.zeros(0, np.int32),
           "edge_graph_index": np.concatenate(egi) if egi else np.zeros(0, np.int32)}
    n_out = out["x"].shape[0]
    out["plan"] = mirror_plan(out["edge_index"], n_out)
    out["plan_t"] = mirror_plan(out["edge_index"][[1, 0]], n_out)
    out["graph_plan"] = mirror_plan(np.stack([out["node_graph_index"], np.arange(n_out, dtype=np.int32)]), len(ids))
    return out


def random_dataset(rng, sizes, F, y=True):
    """Packed arrays of graphs with the given (nodes, edges): random endpoints (self-loops and duplicates happen), random
    weights.  Returns a dict of the from_arrays arguments."""
    node_ptr = np.concatenate([[0], np.cumsum([n for n, _ in sizes])]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum([e for _, e in sizes])]).astype(np.int64)
    ei = [np.stack([rng.integers(0, n, e), rng.integers(0, n, e)]) + off if e else np.zeros((2, 0), np.int64)
          for (n, e), off in zip(sizes, node_ptr[:-1])]
    d = {"x": rng.standard_normal((int(node_ptr[-1]), F)).astype(np.float32),
         "edge_index": np.concatenate(ei, axis=1).astype(np.int32), "node_ptr": node_ptr, "edge_ptr": edge_ptr,
         "edge_weight": rng.uniform(0.5, 1.5, int(edge_ptr[-1])).astype(np.float32)}
    if y:
        d["y"] = rng.integers(0, 7, (len(sizes), 1)).astype(np.int64)
    return d


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_collate_symbols_versions_and_struct_layout():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.COLLATE_SIGNATURES) == ["tfgx_collate", "tfgx_collate_tile", "tfgx_collate_version"]
    for abi in L.ABIS:
        assert abi.signatures is L.COLLATE_SIGNATURES or not any("collate" in n for n in abi.signatures), abi.header
    assert "collate" not in source("tfgx.h")
    from tf_geometric_amd import data
    assert L.load_library().tfgx_collate_tile() == macro(HEADER, "TFGX_COLLATE_TILE") == L.COLLATE_TILE == data.COLLATE_TILE


FAKE = dict(ds_x=1 << 30, ds_ldx=8, F=8, ds_row=2 << 30, ds_col=3 << 30, ds_w=4 << 30, ds_n=100, ds_e=300, table=5 << 30, B=4,
            n_out=50, e_out=120, out_x=6 << 30, out_ldx=8, out_node_graph_index=7 << 30, out_row=8 << 30, out_col=9 << 30,
            out_edge_graph_index=10 << 30, out_w=11 << 30)
FAKE_PLAN = dict(ds_row_ptr=12 << 30, ds_col=13 << 30, ds_perm=14 << 30, out_row_ptr=15 << 30, out_col=16 << 30,
                 out_perm=17 << 30)


def _call(lib, plan=None, plan_t=None, **kw):
    from tf_geometric_amd import _lib as L
    a = L.CollateArgs(**dict(FAKE, **kw))
    keep = []
    for name, p in (("plan", plan), ("plan_t", plan_t)):
        if p is not None:
            keep.append(L.CollatePlan(**p))
            setattr(a, name, ctypes.pointer(keep[-1]))
    return lib.tfgx_collate(ctypes.byref(a), None)


def test_collate_argument_validation_without_gpu():
    """Every refusal returns TFGX_ERR_INVALID_ARG (1) on the host, before any device work (the pointers are not memory), with
    the member named."""
    from tf_geometric_amd import _lib as L
    lib = L.load_library()

    def refused(rc, word):
        assert rc == 1, rc
        assert word in lib.tfgx_last_error(), (word, lib.tfgx_last_error())

    refused(lib.tfgx_collate(None, None), b"args is null")
    for member in ("ds_ldx", "F", "ds_n", "ds_e", "B", "n_out", "e_out", "out_ldx"):
        refused(_call(lib, **{member: -1}), b"negative size (" + member.encode())
        refused(_call(lib, **{member: 1 << 31}), member.encode() + b" = 2147483648 does not fit int32")
    refused(_call(lib, ds_ldx=7), b"ds_ldx = 7 is smaller than F")
    refused(_call(lib, out_ldx=7), b"out_ldx = 7 is smaller than F")
    refused(_call(lib, n_out=401), b"n_out = 401")             # > ds_n * B
    refused(_call(lib, e_out=1201), b"e_out = 1201")           # > ds_e * B
    refused(_call(lib, B=0), b"n_out = 50")                    # no graph can hold a node
    for member in ("table", "ds_x", "out_x", "out_node_graph_index", "ds_row", "ds_col", "out_row", "out_col",
                   "out_edge_graph_index"):
        refused(_call(lib, **{member: None}), member.encode() + b" is null")
    for member in FAKE_PLAN:
        p = dict(FAKE_PLAN, **{member: None})
        refused(_call(lib, plan=p), b"plan->" + member.encode() + b" is null")
        refused(_call(lib, plan_t=p), b"plan_t->" + member.encode() + b" is null")


def test_collate_zero_size_calls_succeed_without_gpu():
    """Without a plan nothing exists to be written, so nothing is launched (with a plan out_row_ptr[0 .. n_out] is written: the
    GPU tests)."""
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    nothing = dict(ds_x=None, ds_row=None, ds_col=None, ds_w=None, table=None, out_x=None, out_node_graph_index=None,
                   out_row=None, out_col=None, out_edge_graph_index=None, out_w=None)
    assert _call(lib, B=0, n_out=0, e_out=0) == 0, lib.tfgx_last_error()
    assert _call(lib, B=0, n_out=0, e_out=0, **nothing) == 0, lib.tfgx_last_error()
    assert _call(lib, B=3, n_out=0, e_out=0, **nothing) == 0, lib.tfgx_last_error()          # three graphs without nodes
    assert _call(lib, B=0, n_out=0, e_out=0, ds_n=0, ds_e=0, F=0, ds_ldx=0, out_ldx=0, **nothing) == 0, lib.tfgx_last_error()


# ---- the mirror ---------------------------------------------------------------------------------------------------------
SIZES = [(3, 4), (0, 0), (5, 0), (2, 6), (1, 1), (0, 0), (7, 20)]


def test_mirror_collate_is_from_graphs_and_its_plans_are_stable_sorts():
    import tf_geometric_amd as tfg
    rng = np.random.Generator(np.random.PCG64(1))
    d = random_dataset(rng, SIZES, 5)
    store = tfg.data.GraphStore.from_arrays(**d)
    for ids in ([0], [6, 3, 3, 0], [1, 0, 5, 1, 2, 4, 1], [1, 5], []):
        m = mirror_collate(d["x"], d["edge_index"], d["edge_weight"], d["node_ptr"], d["edge_ptr"], ids)
        n_out, e_out = m["x"].shape[0], m["edge_index"].shape[1]
        if ids:
            b = tfg.BatchGraph.from_graphs([store.graph(i) for i in ids])
            for key in ("x", "edge_index", "edge_weight", "node_graph_index", "edge_graph_index"):
                assert np.array_equal(m[key], getattr(b, key)) and m[key].dtype == getattr(b, key).dtype, (ids, key)
        row_ptr, col, perm = m["plan"]
        assert row_ptr.shape == (n_out + 1,) and row_ptr[-1] == e_out
        for r in range(n_out):
            p = perm[row_ptr[r]:row_ptr[r + 1]]
            assert (m["edge_index"][0][p] == r).all() and (np.diff(p) > 0).all()
        assert np.array_equal(col, m["edge_index"][1][perm])
        g_row_ptr, g_col, g_perm = m["graph_plan"]
        table, n, e = store.batch_table(ids)
        assert (n, e) == (n_out, e_out)
        assert np.array_equal(g_row_ptr, table[1]) and np.array_equal(g_col, np.arange(n_out)) and np.array_equal(g_perm, g_col)


# ---- GraphStore on the host ---------------------------------------------------------------------------------------------
def test_batch_table_is_the_ptr_arithmetic():
    import tf_geometric_amd as tfg
    rng = np.random.Generator(np.random.PCG64(2))
    d = random_dataset(rng, SIZES, 3)
    store = tfg.data.GraphStore.from_arrays(**d)
    assert len(store) == len(SIZES) and store.num_features == 3
    ids = [6, 1, 2, 6, 5, 0]
    table, n_out, e_out = store.batch_table(np.asarray(ids))
    assert table.dtype == np.int32 and table.shape == (4, len(ids) + 1)
    nodes, edges = [SIZES[i][0] for i in ids], [SIZES[i][1] for i in ids]
    assert n_out == sum(nodes) and e_out == sum(edges)
    assert list(table[0]) == [int(d["node_ptr"][i]) for i in ids] + [0]
    assert list(table[1]) == [sum(nodes[:j]) for j in range(len(ids) + 1)]
    assert list(table[2]) == [int(d["edge_ptr"][i]) for i in ids] + [0]
    assert list(table[3]) == [sum(edges[:j]) for j in range(len(ids) + 1)]
    empty, n0, e0 = store.batch_table([])
    assert empty.shape == (4, 1) and not empty.any() and (n0, e0) == (0, 0)
    g = store.graph(6)
    assert g.num_nodes == 7 and g.num_edges == 20 and g.edge_index.min() >= 0 and g.edge_index.max() < 7
    assert g.edge_index.dtype == np.int32 and g.y.shape == (1, 1)


def test_index_error_before_any_device_work():
    import tf_geometric_amd as tfg
    store = tfg.data.GraphStore.from_arrays(**random_dataset(np.random.Generator(np.random.PCG64(3)), SIZES, 3))
    for ids, word in (([0, 7], "graph id 7"), ([-1], "graph id -1"), (np.asarray([3, 2, 99]), "position 2")):
        with pytest.raises(IndexError, match=word):
            store.batch_table(ids)
        with pytest.raises(IndexError, match=word):          # collate: the same error, with or without a device
            store.collate(ids)
    with pytest.raises(IndexError):
        store.graph(len(SIZES))
    with pytest.raises(IndexError, match="integers"):
        store.batch_table([0.5])


def test_store_refusals_name_the_graph():
    import tf_geometric_amd as tfg
    G = tfg.Graph
    x3 = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError, match=r"graph 1: edge 2 \(1, 3\) has an endpoint outside its 3 nodes"):
        tfg.data.GraphStore([G(x3, [[0], [1]]), G(x3, [[0, 1, 1], [1, 2, 3]])])
    with pytest.raises(ValueError, match=r"graph 0: edge 0 \(-1, 0\)"):
        tfg.data.GraphStore([G(x3, [[-1], [0]])])
    with pytest.raises(ValueError, match="graph 2 has 5 features, graph 0 has 4"):
        tfg.data.GraphStore([G(x3, [[0], [1]]), G(x3, [[0], [1]]), G(np.zeros((2, 5), np.float32), [[0], [1]])])
    # packed arrays: an edge of graph 1 that points into graph 0
    d = random_dataset(np.random.Generator(np.random.PCG64(4)), [(3, 2), (4, 3)], 2, y=False)
    d["edge_index"][1, 3] = 2
    with pytest.raises(ValueError, match=r"graph 1: edge 1 \(\d, -1\) has an endpoint outside its 4 nodes"):
        tfg.data.GraphStore.from_arrays(**d)
    # totals beyond int32: the ptr arrays alone decide, before the arrays are looked at
    big = np.asarray([0, 1 << 30, 1 << 31], dtype=np.int64)
    with pytest.raises(ValueError, match="graph 1: the dataset's nodes .* do not fit int32"):
        tfg.data.GraphStore.from_arrays(np.zeros((0, 2), np.float32), np.zeros((2, 0), np.int32), big, np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="graph 1: the dataset's edges .* do not fit int32"):
        tfg.data.GraphStore.from_arrays(np.zeros((0, 2), np.float32), np.zeros((2, 0), np.int32), np.zeros(3, np.int64), big)
    with pytest.raises(ValueError, match="graph 1: y must have one leading row"):
        tfg.data.GraphStore([G(x3, [[0], [1]], y=[1]), G(x3, [[0], [1]], y=[1, 2])])


def test_collate_needs_a_gpu():
    import torch
    import tf_geometric_amd as tfg
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the refusal cannot be observed")
    store = tfg.data.GraphStore.from_arrays(**random_dataset(np.random.Generator(np.random.PCG64(5)), SIZES, 3))
    with pytest.raises(tfg._lib.TfgxError):
        store.collate([0, 1])
