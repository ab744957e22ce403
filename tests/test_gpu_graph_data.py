# coding=utf-8
"""The methods of tfg.Graph / tfg.BatchGraph that go over device operators: adj(), to_directed() (edge_graph_index merged with
"max"), sample_new_graph_by_node_index(), on numpy graphs (numpy out) and on device graphs (tensors out), against results
written out by hand."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _graph(tfg):
    """Three nodes, the edge (0, 1) twice (once as (1, 0)) and (1, 2): weights 1, 2, 3."""
    x = np.arange(6, dtype=np.float32).reshape(3, 2)
    return tfg.Graph(x, [[0, 1, 1], [1, 0, 2]], y=[10, 11, 12], edge_weight=[1.0, 2.0, 3.0])


def test_adj_is_the_sparse_matrix_of_the_graph(tfg):
    g = _graph(tfg)
    a = g.adj()
    assert isinstance(a, tfg.SparseMatrix) and a.shape == [3, 3]
    dense = np.zeros((3, 3), np.float32)
    dense[g.edge_index[0], g.edge_index[1]] = g.edge_weight
    assert np.allclose(_np(a.matmul(torch.from_numpy(g.x).cuda())), dense @ g.x)


@pytest.mark.parametrize("device_graph", [False, True], ids=["numpy", "tensor"])
def test_to_directed(tfg, device_graph):
    g = _graph(tfg)
    b = tfg.BatchGraph.from_graphs([g, g])
    if device_graph:
        g, b = g.convert_data_to_tensor(), b.convert_data_to_tensor()
    kind = torch.Tensor if device_graph else np.ndarray
    d = g.to_directed()
    assert d is not g and isinstance(d.edge_index, kind) and isinstance(d.edge_weight, kind)
    assert _np(d.edge_index).tolist() == [[0, 1, 1, 2], [1, 2, 0, 1]] and _np(d.edge_weight).tolist() == [3.0, 3.0, 3.0, 3.0]
    assert _np(g.edge_index).shape == (2, 3) and _np(d.y).tolist() == [10, 11, 12]
    assert _np(g.to_directed(merge_mode="max").edge_weight).tolist() == [2.0, 3.0, 2.0, 3.0]
    db = b.to_directed()
    assert isinstance(db, tfg.BatchGraph) and db.num_graphs == 2 and isinstance(db.edge_graph_index, kind)
    assert _np(db.edge_index).tolist() == [[0, 1, 3, 4, 1, 2, 4, 5], [1, 2, 4, 5, 0, 1, 3, 4]]
    assert _np(db.edge_graph_index).tolist() == [0, 0, 1, 1, 0, 0, 1, 1] and _np(db.edge_graph_index).dtype == np.int32
    assert _np(db.edge_weight).tolist() == [3.0] * 8 and _np(db.node_graph_index).tolist() == [0, 0, 0, 1, 1, 1]
    with pytest.warns(DeprecationWarning, match="to_directed.inplace=True."):
        assert b.convert_edge_to_directed() is b                       # the deprecated spelling works in place
    assert _np(b.edge_index).shape == (2, 8) and _np(b.edge_graph_index).tolist() == [0, 0, 1, 1, 0, 0, 1, 1]


@pytest.mark.parametrize("device_graph", [False, True], ids=["numpy", "tensor"])
def test_sample_new_graph_by_node_index(tfg, device_graph):
    ring = tfg.Graph(np.arange(8, dtype=np.float32).reshape(4, 2), [[0, 1, 2, 3], [1, 2, 3, 0]], y=[20, 21, 22, 23],
                     edge_weight=[1.0, 2.0, 3.0, 4.0])
    b = tfg.BatchGraph.from_graphs([ring, ring])
    b.y = np.arange(8)                                                   # one row per node: gathered with the nodes
    if device_graph:
        ring, b = ring.convert_data_to_tensor(), b.convert_data_to_tensor()
    index = [3, 1, 2]
    index = torch.tensor(index, device="cuda") if device_graph else np.asarray(index)
    s = ring.sample_new_graph_by_node_index(index)
    assert type(s) is tfg.Graph and isinstance(s.edge_index, torch.Tensor if device_graph else np.ndarray)
    assert _np(s.x).tolist() == [[6.0, 7.0], [2.0, 3.0], [4.0, 5.0]] and _np(s.y).tolist() == [23, 21, 22]
    assert _np(s.edge_index).tolist() == [[1, 2], [2, 0]] and _np(s.edge_weight).tolist() == [2.0, 3.0]       # (1, 2), (2, 3)
    index = [6, 0, 1, 5]                                                 # (0, 1) of the first ring, (5, 6) of the second
    index = torch.tensor(index, device="cuda") if device_graph else np.asarray(index)
    sb = b.sample_new_graph_by_node_index(index)
    assert isinstance(sb, tfg.BatchGraph) and _np(sb.node_graph_index).tolist() == [1, 0, 0, 1]
    assert _np(sb.edge_index).tolist() == [[1, 3], [2, 0]] and _np(sb.edge_graph_index).tolist() == [0, 1]
    assert _np(sb.edge_weight).tolist() == [1.0, 2.0] and _np(sb.y).tolist() == [6, 0, 1, 5] and sb.num_graphs == 2
