# coding=utf-8
"""tfg.Graph / tfg.BatchGraph without a GPU: the numpy paths equal tests/golden/batch_graph_cases.npz — what the reference's own
casts and BatchGraph.from_graphs give on the cases of tests/batch_graph_cases.py — exactly, dtypes included (re-run live where
the reference checkout exists); properties, __repr__, the lazy x, the deprecation warning; the two stated deviations from the
reference (num_graphs, to_graphs with a per-graph y); and to_graphs(from_graphs(gs)) returns the graphs."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT
import batch_graph_cases as bc

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_batch_graph_golden as mk     # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "batch_graph_cases.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _same(got, ref, what):
    assert isinstance(got, np.ndarray), what
    assert got.dtype == ref.dtype and got.shape == ref.shape, "{}: {} {} vs {} {}".format(what, got.dtype, got.shape, ref.dtype,
                                                                                        ref.shape)
    assert np.array_equal(got, ref), what


def test_golden_file_is_small():
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_numpy_paths_equal_the_reference_exactly(name, golden):
    import tf_geometric_amd as tfg
    assert str(golden[name + "::__inputs_sha256__"]) == mk.inputs_digest(bc.CASES[name]()), "the case table changed"
    outs = bc.run(tfg.Graph, tfg.BatchGraph, bc.CASES[name]())
    keys = [k for k in golden if k.startswith(name + "::") and not k.endswith("__")]
    assert sorted(keys) == sorted(name + "::" + k for k in outs)
    for k, v in outs.items():
        _same(v, golden[name + "::" + k], "{} {}".format(name, k))


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_golden_file_is_what_the_reference_produces(name, golden):
    from oracle.ref_harness import reference_available
    if not reference_available():
        pytest.skip("reference checkout not present")
    outs = mk.run_reference(name)
    keys = [k for k in golden if k.startswith(name + "::") and not k.endswith("__")]
    assert sorted(keys) == sorted(name + "::" + k for k in outs)
    for k, v in outs.items():
        _same(np.asarray(v), golden[name + "::" + k], "{} {}: live reference run differs from the golden file".format(name, k))


def _graphs(name="all_weights_y_f32"):
    import tf_geometric_amd as tfg
    return [tfg.Graph(**g) for g in bc.CASES[name]()]


def test_exports_and_casts():
    import tf_geometric_amd as tfg
    assert tfg.Graph is tfg.data.Graph and tfg.BatchGraph is tfg.data.BatchGraph and issubclass(tfg.BatchGraph, tfg.Graph)
    g = tfg.Graph([[1.0, 2.0], [3.0, 4.0]], [[0, 1], [1, 0]], y=[1, 0], edge_weight=[0.5, 2])
    assert g.x.dtype == np.float32 and g.edge_index.dtype == np.int32 and g.edge_weight.dtype == np.float32
    assert isinstance(g.y, np.ndarray) and g.y.dtype == np.asarray([1, 0]).dtype and g.cache == {}
    assert (g.num_nodes, g.num_edges, g.num_features) == (2, 2, 2)
    assert tfg.Graph(np.zeros((4, 2), np.float16), []).x.dtype == np.float16          # only float64 is down-cast
    # tensors: float64 -> float32, indices -> int32, weights default to ones on the index's device
    t = tfg.Graph(torch.zeros(3, 2, dtype=torch.float64), torch.tensor([[0, 1], [1, 2]]), edge_weight=torch.ones(2, dtype=torch.float64))
    assert t.x.dtype == torch.float32 and t.edge_index.dtype == torch.int32 and t.edge_weight.dtype == torch.float32
    d = tfg.Graph(torch.zeros(3, 2), torch.tensor([[0, 1], [1, 2]]))
    assert isinstance(d.edge_weight, torch.Tensor) and torch.equal(d.edge_weight, torch.ones(2)) and d.num_edges == 2


def test_empty_edge_lists_count_zero_edges():
    import tf_geometric_amd as tfg
    x = np.zeros((3, 2), np.float32)
    for empty in ([], np.zeros((2, 0), np.int64), np.zeros(0, np.int32), torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0)):
        g = tfg.Graph(x, empty)
        assert g.num_edges == 0 and tuple(g.edge_weight.shape) == (0,) and g.edge_weight.dtype in (np.float32, torch.float32)


def test_repr_and_shape_desc():
    import tf_geometric_amd as tfg
    g = tfg.Graph(np.zeros((3, 2), np.float32), [[0, 1], [1, 2]], y=[7])
    assert g.get_shape_desc() == "Graph Shape: x => (3, 2)\tedge_index => (2, 2)\ty => (1,)" == str(g) == repr(g)
    assert "y => None" in repr(tfg.Graph(np.zeros((3, 2), np.float32), [[0], [1]]))
    b = tfg.BatchGraph.from_graphs([g, g])
    assert repr(b) == "Graph Shape: x => (6, 2)\tedge_index => (2, 4)\ty => (2,)"


def test_x_may_be_a_function():
    import tf_geometric_amd as tfg
    calls = []

    def make_x():
        calls.append(1)
        return np.full((4, 3), len(calls), np.float32)

    g = tfg.Graph(make_x, [[0, 1], [1, 2]])
    assert calls == []                                   # nothing is evaluated at construction (weights come from the edges)
    assert g.num_nodes == 4 and g.num_features == 3 and g.x[0, 0] == 3.0 and len(calls) == 3          # every access calls it
    c = g.convert_data_to_tensor()
    assert c._x is make_x and isinstance(c.edge_index, torch.Tensor)          # the function itself stays (:216)
    assert not isinstance(tfg.Graph(np.zeros, [[0], [0]])._x, np.ndarray)     # a builtin is not a FunctionType: kept as given


def test_convert_data_to_tensor():
    import tf_geometric_amd as tfg
    g = _graphs()[0]
    c = g.convert_data_to_tensor()
    assert c is not g and isinstance(g.x, np.ndarray)
    for key in ("x", "edge_index", "edge_weight", "y"):
        t = getattr(c, key)
        assert isinstance(t, torch.Tensor) and np.array_equal(t.cpu().numpy(), getattr(g, key)), key
    assert c.x.is_cuda == torch.cuda.is_available()
    assert g.convert_data_to_tensor(inplace=True) is g and isinstance(g.x, torch.Tensor)
    b = tfg.BatchGraph.from_graphs(_graphs())
    cb = b.convert_data_to_tensor()
    assert isinstance(cb, tfg.BatchGraph) and cb.num_graphs == 5 and cb.graphs is b.graphs
    assert isinstance(cb.node_graph_index, torch.Tensor) and cb.node_graph_index.dtype == torch.int32
    assert np.array_equal(cb.edge_graph_index.cpu().numpy(), b.edge_graph_index)
    nb = tfg.BatchGraph(b.x, b.edge_index, b.node_graph_index, b.edge_graph_index).convert_data_to_tensor()
    assert nb.y is None and nb.num_graphs == 5 - 0           # hand-made: max + 1 = 5 (graph 4 has a node)


def test_deprecated_spelling_warns():
    import tf_geometric_amd as tfg
    g = tfg.Graph(np.zeros((2, 2), np.float32), [[0], [1]])
    b = tfg.BatchGraph.from_graphs([g])
    for obj, word in ((g, "'Graph.convert_edge_to_directed"), (b, "'BatchGraph.convert_edge_to_directed")):
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            try:
                obj.convert_edge_to_directed()
            except tfg._lib.TfgxError:
                assert not torch.cuda.is_available()          # the merge itself runs on the GPU; the warning comes first
        assert [w for w in seen if issubclass(w.category, DeprecationWarning) and word in str(w.message)
                and "to_directed(inplace=True)" in str(w.message)], [str(w.message) for w in seen]


# ---- the two deviations ---------------------------------------------------------------------------------------------------
def test_num_graphs_counts_trailing_empty_graphs():
    import tf_geometric_amd as tfg
    g = tfg.Graph(np.zeros((2, 3), np.float32), [[0], [1]])
    e = tfg.Graph(np.zeros((0, 3), np.float32), np.zeros((2, 0), np.int32))
    b = tfg.BatchGraph.from_graphs([e, g, e, e])
    assert b.num_graphs == 4 and list(b.node_graph_index) == [1, 1]
    hand = tfg.BatchGraph(b.x, b.edge_index, b.node_graph_index, b.edge_graph_index)
    assert hand.num_graphs == 2                           # the reference's rule: max(node_graph_index) + 1
    assert tfg.BatchGraph(b.x, b.edge_index, torch.from_numpy(b.node_graph_index), b.edge_graph_index).num_graphs == 2
    assert tfg.BatchGraph(np.zeros((0, 3), np.float32), np.zeros((2, 0), np.int32), np.zeros(0, np.int32),
                          np.zeros(0, np.int32)).num_graphs == 0
    assert len(b.to_graphs()) == 4 and len(hand.to_graphs()) == 2


def _assert_graphs_equal(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for key in ("x", "edge_index", "edge_weight", "y"):
            u, v = getattr(a, key), getattr(b, key)
            if v is None:
                assert u is None, key
            else:
                _same(np.asarray(u), np.asarray(v), key)


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_to_graphs_returns_the_graphs(name):
    """Per-graph y ([1] / [1, 3] rows), absent y, empty graphs in the middle and a one-node graph at the end."""
    import tf_geometric_amd as tfg
    gs = _graphs(name)
    b = tfg.BatchGraph.from_graphs(gs)
    _assert_graphs_equal(b.to_graphs(), gs)
    # shuffled edges: reorder() sorts them back by graph, stably (nodes are not renumbered, as in the reference, so the node
    # order stays the batch's)
    pe = np.random.Generator(np.random.PCG64(9)).permutation(b.num_edges)
    s = tfg.BatchGraph(b.x, b.edge_index[:, pe], b.node_graph_index, b.edge_graph_index[pe], y=b.y, edge_weight=b.edge_weight[pe])
    s._num_graphs = 5
    for a, g in zip(s.to_graphs(), gs):
        _same(np.asarray(a.x), np.asarray(g.x), "x")
        assert a.num_edges == g.num_edges

        def triples(gr):
            return sorted(zip(gr.edge_index[0].tolist(), gr.edge_index[1].tolist(), gr.edge_weight.tolist()))

        assert triples(a) == triples(g)


def test_to_graphs_splits_y_per_node_per_graph_or_refuses():
    import tf_geometric_amd as tfg
    gs = _graphs("f32_no_weights_no_y")
    b = tfg.BatchGraph.from_graphs(gs)                     # 11 nodes, 5 graphs
    per_node = np.arange(11, dtype=np.int64) * 10
    b.y = per_node
    parts = [g.y for g in b.to_graphs()]
    assert [len(p) for p in parts] == [3, 0, 5, 2, 1] and np.array_equal(np.concatenate(parts), per_node)
    b.y = np.arange(5, dtype=np.float32).reshape(5, 1)
    assert [g.y.tolist() for g in b.to_graphs()] == [[[0.0]], [[1.0]], [[2.0]], [[3.0]], [[4.0]]]
    assert np.array_equal(b.reorder().y, b.y)             # a per-graph y is not gathered with the node order
    for rows in (4, 6, 12):
        b.y = np.zeros((rows, 2))
        with pytest.raises(ValueError, match="neither one per node .11. nor one per graph .5."):
            b.to_graphs()
    b.y = np.float32(3.0)                                  # a scalar: refused as well
    with pytest.raises(ValueError):
        b.to_graphs()


def test_tensor_graphs_are_joined_with_torch_cat():
    import tf_geometric_amd as tfg
    gs = _graphs()
    ts = [tfg.Graph(torch.from_numpy(g.x), torch.from_numpy(g.edge_index), y=torch.from_numpy(g.y),
                    edge_weight=torch.from_numpy(g.edge_weight)) for g in gs]
    b, t = tfg.BatchGraph.from_graphs(gs), tfg.BatchGraph.from_graphs(ts)
    for key in ("x", "edge_index", "node_graph_index", "edge_graph_index", "edge_weight", "y"):
        v = getattr(t, key)
        assert isinstance(v, torch.Tensor) and v.dtype == torch.from_numpy(getattr(b, key)).dtype, key
        assert np.array_equal(v.numpy(), getattr(b, key)), key
    assert t.num_graphs == 5
    _assert_graphs_equal([tfg.Graph(g.x.numpy(), g.edge_index.numpy(), g.y.numpy(), g.edge_weight.numpy()) for g in t.to_graphs()], gs)
