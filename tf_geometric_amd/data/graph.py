# coding=utf-8
"""Graph / BatchGraph: the containers every graph-classification demo of the reference starts from
(tf_geometric/data/graph.py:20-620), with torch tensors where the reference has TF tensors and numpy kept as numpy.
tensor_spec_* is TensorFlow-only and is left out; sparse x is not supported."""
import types
import warnings

import numpy as np
import torch

from .. import _lib as L


def _get_shape(data):
    return None if data is None else tuple(data.shape)


def _is_tensor(data):
    return isinstance(data, torch.Tensor)


def _tensor_device():
    """Where convert_data_to_tensor puts data: the current GPU; without one the containers still work, on CPU tensors (the
    operators that take them do not: _lib.require_gpu)."""
    return L.device() if torch.cuda.is_available() else torch.device("cpu")


def _take(data, index):
    """data[index] along the first axis for numpy and tensors alike."""
    if _is_tensor(data):
        return data.index_select(0, torch.as_tensor(index, device=data.device).long())
    return np.asarray(data)[np.asarray(index)]


class Graph(object):
    """
    A Graph object wrappers all the data of a graph,
    including node features, edge info (index and weight) and graph label
    """

    def __init__(self, x, edge_index, y=None, edge_weight=None):
        """
        :param x: Tensor/NDArray/list, shape: [num_nodes, num_features], node features, or a zero-argument function
            that returns them (evaluated at every access of ``graph.x``, :139-143).
        :param edge_index: Tensor/NDArray/list, shape: [2, num_edges].  Each column (u, v) is a directed edge.
        :param y: Tensor/NDArray/list/None, any shape, graph label.  To build a BatchGraph out of graphs, y cannot be a scalar.
        :param edge_weight: Tensor/NDArray/list/None, shape: [num_edges]; ones when absent (:50-56).
        """
        self._x = Graph.cast_x(x)
        self.edge_index = Graph.cast_edge_index(edge_index)
        self.y = Graph.cast_y(y)
        self.cache = {}

        if edge_weight is not None:
            self.edge_weight = self.cast_edge_weight(edge_weight)
        elif _is_tensor(self.edge_index):
            self.edge_weight = torch.ones([self.num_edges], dtype=torch.float32, device=self.edge_index.device)
        else:
            self.edge_weight = np.ones([self.num_edges], dtype=np.float32)

    @classmethod
    def cast_edge_index(cls, x):
        if isinstance(x, list):
            x = np.array(x).astype(np.int32)
        elif isinstance(x, np.ndarray):
            x = x.astype(np.int32)
        elif _is_tensor(x):
            x = x.to(torch.int32)
        return x

    @classmethod
    def cast_edge_weight(cls, edge_weight):
        if isinstance(edge_weight, list):
            edge_weight = np.array(edge_weight).astype(np.float32)
        elif isinstance(edge_weight, np.ndarray):
            edge_weight = edge_weight.astype(np.float32)
        elif _is_tensor(edge_weight) and not isinstance(edge_weight, torch.nn.Parameter):
            edge_weight = edge_weight.to(torch.float32)
        return edge_weight

    @classmethod
    def cast_x(cls, x):
        if isinstance(x, list):
            x = np.array(x)
        if isinstance(x, np.ndarray) and x.dtype == np.float64:
            x = x.astype(np.float32)
        elif _is_tensor(x) and not isinstance(x, torch.nn.Parameter) and x.dtype == torch.float64:
            x = x.to(torch.float32)
        return x

    @classmethod
    def cast_y(cls, y):
        if isinstance(y, list):
            y = np.array(y)
        return y

    @property
    def x(self):
        if isinstance(self._x, types.FunctionType):
            return self._x()
        return self._x

    @property
    def num_nodes(self):
        return len(self.x)

    @property
    def num_edges(self):
        """Number of edges; 0 for an empty list (``[]`` or shape [0]) as well as for shape [2, 0]."""
        if _is_tensor(self.edge_index):
            return 0 if self.edge_index.shape[0] == 0 else int(self.edge_index.shape[1])
        if len(self.edge_index) == 0:
            return 0
        return len(self.edge_index[0])

    @property
    def num_features(self):
        return self.x.shape[-1]

    def get_shape_desc(self):
        return "Graph Shape: x => {}\tedge_index => {}\ty => {}".format(
            _get_shape(self.x), _get_shape(self.edge_index), _get_shape(self.y))

    def __str__(self):
        return self.get_shape_desc()

    def __repr__(self):
        return self.__str__()

    def adj(self):
        """The [num_nodes, num_nodes] adjacency as this package's SparseMatrix (tf_sparse.SparseMatrix in the reference)."""
        from ..sparse import SparseMatrix
        num_nodes = self.num_nodes
        return SparseMatrix(self.edge_index, self.edge_weight, shape=[num_nodes, num_nodes])

    def _inplace_convert_data_to_tensor(self, keys):
        dev = _tensor_device()
        for key in keys:
            data = getattr(self, key)
            if data is not None and not _is_tensor(data) and not isinstance(data, types.FunctionType):
                setattr(self, key, torch.from_numpy(np.ascontiguousarray(np.asarray(data))).to(dev))
        return self

    def convert_data_to_tensor(self, inplace=False):
        """Convert all graph data into device tensors.  inplace=False returns a new Graph and leaves this one alone."""
        if inplace:
            graph = self
        else:
            graph = Graph(self._x, self.edge_index, y=self.y, edge_weight=self.edge_weight)
        graph._inplace_convert_data_to_tensor(["_x", "edge_index", "edge_weight", "y"])
        return graph

    def to_directed(self, merge_mode="sum", inplace=False):
        """(u, v) -> (u, v) and (v, u), duplicates merged with `merge_mode` (tfg.utils.convert_edge_to_directed).

        :return: If inplace is False, a new graph with directed edges; else this graph, changed."""
        from ..utils import convert_edge_to_directed
        edge_index, [edge_weight] = convert_edge_to_directed(self.edge_index, [self.edge_weight], merge_modes=[merge_mode])
        if inplace:
            self.edge_index, self.edge_weight = edge_index, edge_weight
            return self
        return Graph(self.x, edge_index, y=self.y, edge_weight=edge_weight)

    def convert_edge_to_directed(self, merge_mode="sum"):
        """.. deprecated:: Use ``to_directed(inplace=True)`` instead."""
        warnings.warn(
            "'Graph.convert_edge_to_directed(self, merge_mode)' is deprecated, use 'Graph.to_directed(inplace=True)' instead",
            DeprecationWarning)
        return self.to_directed(merge_mode, inplace=True)

    def sample_new_graph_by_node_index(self, sampled_node_index):
        """A new graph of the nodes in `sampled_node_index` (renumbered by their position in it) and the edges between them
        (tfg.utils.sample_new_graph_by_node_index); x, y and, for a BatchGraph, node_graph_index are gathered per node."""
        from ..utils import sample_new_graph_by_node_index
        is_batch_graph = isinstance(self, BatchGraph)
        x, edge_index, edge_weight, node_graph_index = sample_new_graph_by_node_index(
            self.edge_index, sampled_node_index, x=self.x, edge_weight=self.edge_weight,
            node_graph_index=self.node_graph_index if is_batch_graph else None)
        idx = sampled_node_index.cpu().numpy() if _is_tensor(sampled_node_index) else np.asarray(sampled_node_index)
        y = None if self.y is None else _take(self.y, idx)
        if not is_batch_graph:
            return Graph(x=x, edge_index=edge_index, y=y, edge_weight=edge_weight)
        # an edge lies inside one graph: its graph is the graph of its first endpoint
        if _is_tensor(edge_index):
            edge_graph_index = torch.as_tensor(node_graph_index, device=edge_index.device).to(torch.int32)[edge_index[0].long()]
        else:
            ngi = node_graph_index.cpu().numpy() if _is_tensor(node_graph_index) else np.asarray(node_graph_index)
            edge_graph_index = ngi.astype(np.int32)[edge_index[0]]
        return BatchGraph(x=x, edge_index=edge_index, node_graph_index=node_graph_index, edge_graph_index=edge_graph_index,
                          y=y, edge_weight=edge_weight)


class BatchGraph(Graph):
    """
    Batch graph wrap a batch of graphs into a single graph, where each nodes has an unique index and a graph index.
    The node_graph_index is the index of the corresponding graph for each node in the batch.
    The edge_graph_index is the index of the corresponding graph for each edge in the batch.

    Two deviations from the reference:

    - ``num_graphs``: a batch made by ``from_graphs`` or by ``GraphStore.collate`` knows its graph count, so trailing graphs
      without nodes are counted.  Only a hand-constructed batch falls back to ``max(node_graph_index) + 1`` (the reference's
      rule everywhere).
    - ``to_graphs`` / ``reorder``: ``y`` is split per node when it has ``num_nodes`` rows and per graph when it has
      ``num_graphs != num_nodes`` rows; anything else raises ``ValueError``.  (The reference gathers every ``y`` with the node
      sort index, which for the per-graph ``y`` that ``from_graphs`` itself produces is an index error.)
    """

    def __init__(self, x, edge_index, node_graph_index, edge_graph_index, y=None, edge_weight=None, graphs=None):
        super().__init__(x, edge_index, y, edge_weight)
        self.node_graph_index = node_graph_index
        self.edge_graph_index = edge_graph_index
        self.graphs = graphs
        self._num_graphs = None if graphs is None else len(graphs)

    @property
    def num_graphs(self):
        if self._num_graphs is not None:
            return self._num_graphs
        if len(self.node_graph_index) == 0:
            return 0
        if _is_tensor(self.node_graph_index):
            return int(self.node_graph_index.max().item()) + 1
        return int(np.max(self.node_graph_index)) + 1

    def _y_rows(self, num_graphs):
        """"node" / "graph" / None: how y is laid out (see the class docstring)."""
        if self.y is None:
            return None
        rows = int(self.y.shape[0]) if len(self.y.shape) > 0 else -1
        if rows == self.num_nodes:
            return "node"
        if rows == num_graphs:
            return "graph"
        raise ValueError("y has {} rows: neither one per node ({}) nor one per graph ({})".format(
            max(rows, 0), self.num_nodes, num_graphs))

    def reorder(self):
        """Nodes and edges sorted (stably) by their graph index.  A per-node y follows the nodes, a per-graph y stays."""
        num_graphs = self.num_graphs
        if _is_tensor(self.node_graph_index):
            node_sort_index = torch.argsort(self.node_graph_index.long(), stable=True)
        else:
            node_sort_index = np.argsort(np.asarray(self.node_graph_index), kind="stable")
        if _is_tensor(self.edge_graph_index):
            edge_sort_index = torch.argsort(self.edge_graph_index.long(), stable=True)
        else:
            edge_sort_index = np.argsort(np.asarray(self.edge_graph_index), kind="stable")

        def to_index(index, like):      # an index of the kind `like` understands
            if _is_tensor(like):
                return torch.as_tensor(index, device=like.device)
            return index.cpu().numpy() if _is_tensor(index) else index

        node_graph_index = _take(self.node_graph_index, to_index(node_sort_index, self.node_graph_index))
        x = _take(self.x, to_index(node_sort_index, self.x))
        y = self.y
        if self._y_rows(num_graphs) == "node":
            y = _take(self.y, to_index(node_sort_index, self.y))
        edge_graph_index = _take(self.edge_graph_index, to_index(edge_sort_index, self.edge_graph_index))
        es = to_index(edge_sort_index, self.edge_index)
        edge_index = self.edge_index.index_select(1, es.long()) if _is_tensor(self.edge_index) else self.edge_index[:, es]
        edge_weight = None if self.edge_weight is None else _take(self.edge_weight, to_index(edge_sort_index, self.edge_weight))
        batch = BatchGraph(x, edge_index, node_graph_index, edge_graph_index, y=y, edge_weight=edge_weight)
        batch._num_graphs = num_graphs
        return batch

    def to_graphs(self):
        batch_graph = self.reorder()
        num_graphs = batch_graph.num_graphs
        y_rows = batch_graph._y_rows(num_graphs)

        def host(index):
            return index.cpu().numpy() if _is_tensor(index) else np.asarray(index)

        num_nodes_list = np.bincount(host(batch_graph.node_graph_index).astype(np.int64), minlength=num_graphs)
        num_edges_list = np.bincount(host(batch_graph.edge_graph_index).astype(np.int64), minlength=num_graphs)
        nodes_before = np.concatenate([[0], np.cumsum(num_nodes_list)]).astype(np.int64).tolist()
        edges_before = np.concatenate([[0], np.cumsum(num_edges_list)]).astype(np.int64).tolist()

        graphs = []
        for i in range(num_graphs):
            x = batch_graph.x[nodes_before[i]: nodes_before[i + 1]]
            if y_rows is None:
                y = None
            elif y_rows == "node":
                y = batch_graph.y[nodes_before[i]: nodes_before[i + 1]]
            else:
                y = batch_graph.y[i: i + 1]
            edge_index = batch_graph.edge_index[:, edges_before[i]:edges_before[i + 1]] - nodes_before[i]
            edge_weight = None if batch_graph.edge_weight is None else batch_graph.edge_weight[edges_before[i]:edges_before[i + 1]]
            graphs.append(Graph(x=x, edge_index=edge_index, y=y, edge_weight=edge_weight))
        return graphs

    @classmethod
    def from_graphs(cls, graphs):
        """numpy graphs give numpy arrays, array for array what the reference gives; tensor graphs are joined with torch.cat."""
        return BatchGraph(x=BatchGraph.build_x(graphs), edge_index=BatchGraph.build_edge_index(graphs),
                          node_graph_index=BatchGraph.build_node_graph_index(graphs),
                          edge_graph_index=BatchGraph.build_edge_graph_index(graphs), graphs=graphs,
                          y=BatchGraph.build_y(graphs), edge_weight=BatchGraph.build_edge_weight(graphs))

    @classmethod
    def _build_graph_index(cls, graphs, counts):
        first = graphs[0].edge_index
        if _is_tensor(first):
            return torch.cat([torch.full([c], i, dtype=torch.int32, device=first.device) for i, c in enumerate(counts)], dim=0)
        return np.concatenate([np.full([c], i, dtype=np.int32) for i, c in enumerate(counts)], axis=0)

    @classmethod
    def build_node_graph_index(cls, graphs):
        return cls._build_graph_index(graphs, [graph.num_nodes for graph in graphs])

    @classmethod
    def build_edge_graph_index(cls, graphs):
        return cls._build_graph_index(graphs, [graph.num_edges for graph in graphs])

    @classmethod
    def _concat(cls, parts, axis=0):
        if _is_tensor(parts[0]):
            return torch.cat(parts, dim=axis)
        return np.concatenate(parts, axis=axis)

    @classmethod
    def build_x(cls, graphs):
        return cls._concat([graph.x for graph in graphs])

    @classmethod
    def build_edge_index(cls, graphs):
        edge_index_list = []
        num_history_nodes = 0
        for graph in graphs:
            edge_index_list.append(graph.edge_index + num_history_nodes)
            num_history_nodes += graph.num_nodes
        return cls._concat(edge_index_list, axis=1)

    @classmethod
    def build_edge_weight(cls, graphs):
        if graphs[0].edge_weight is None:
            return None
        return cls._concat([graph.edge_weight for graph in graphs])

    @classmethod
    def build_y(cls, graphs):
        if graphs[0].y is None:
            return None
        return cls._concat([graph.y for graph in graphs])

    def convert_data_to_tensor(self, inplace=False):
        """Convert all graph data into device tensors.  inplace=False returns a new BatchGraph and leaves this one alone."""
        if inplace:
            graph = self
        else:
            graph = BatchGraph(self._x, self.edge_index, self.node_graph_index, self.edge_graph_index, y=self.y,
                               edge_weight=self.edge_weight, graphs=self.graphs)
            graph._num_graphs = self._num_graphs
        return graph._inplace_convert_data_to_tensor(["_x", "edge_index", "edge_weight", "y", "node_graph_index",
                                                      "edge_graph_index"])

    def to_directed(self, merge_mode="sum", inplace=False):
        """As Graph.to_directed; edge_graph_index is merged with "max" (all copies of an edge lie in one graph)."""
        from ..utils import convert_edge_to_directed
        edge_index, [edge_weight, edge_graph_index] = convert_edge_to_directed(
            self.edge_index, [self.edge_weight, self.edge_graph_index], merge_modes=[merge_mode, "max"])
        # the merge runs in float32: graph ids come back as exact small floats
        if _is_tensor(edge_graph_index):
            edge_graph_index = edge_graph_index.to(torch.int32)
        else:
            edge_graph_index = np.asarray(edge_graph_index).astype(np.int32)
        if inplace:
            self.edge_index, self.edge_weight, self.edge_graph_index = edge_index, edge_weight, edge_graph_index
            return self
        batch = BatchGraph(self.x, edge_index, self.node_graph_index, edge_graph_index, y=self.y, edge_weight=edge_weight)
        batch._num_graphs = self._num_graphs
        return batch

    def convert_edge_to_directed(self, merge_mode="sum"):
        """.. deprecated:: Use ``to_directed(inplace=True)`` instead."""
        warnings.warn(
            "'BatchGraph.convert_edge_to_directed(self, merge_mode)' is deprecated, use 'BatchGraph.to_directed(inplace=True)' instead",
            DeprecationWarning)
        return self.to_directed(merge_mode, inplace=True)


class StaticBatchGraph(BatchGraph):
    """What ``GraphStore.collate_static`` returns: a batch of ``B`` slots at sizes the host knows (``capacities``), with inert
    padding.  ``num_graphs == B + 1``: slot ``B`` is the dead graph that owns every padded row.  ``graph_mask`` bool [B] says
    which slots are live; ``counts`` int32 [4] on the device holds live graphs, live nodes, live edges and the flags
    ``check()`` reads.  ``y`` has one row per slot; a dead slot holds graph 0's label, so mask it:

        h = gcn1([b.x, b.edge_index, b.edge_weight], cache=b.cache, training=True)
        logits = dense(b.readout(h, "mean"))
        per_slot = cross_entropy(logits, b.y.reshape(-1), reduction="none")
        loss = torch.where(b.graph_mask, per_slot, 0.0).sum() / b.counts[0].clamp(min=1)

    Nothing here reads the device back except ``check()``."""

    _READOUTS = ("mean", "sum", "max", "min")

    def __init__(self, x, edge_index, node_graph_index, edge_graph_index, y, edge_weight, ids, graph_mask, counts, capacities,
                 store_len, given_ids=None):
        super().__init__(x, edge_index, node_graph_index, edge_graph_index, y=y, edge_weight=edge_weight)
        self.ids = ids                  # int32 [B], as the kernel read them (an id beyond int32 held to an out-of-range one)
        self._given_ids = ids if given_ids is None else given_ids
        self.graph_mask = graph_mask
        self.counts = counts
        self.capacities = capacities
        self.num_slots = int(graph_mask.shape[0])
        self._num_graphs = self.num_slots + 1
        self._store_len = int(store_len)
        self._store = None              # the GraphStore behind the batch (collate_static sets it; a pooled batch hands it on)
        self.graph_row_ptr = None       # int32 [B + 2]: the slots' row offsets, the live total, n_cap (the graph plan's row_ptr)
        self.node_index = None          # a pooled batch (nn.sag_pool_static): pooled row -> parent row, -1 for a dead row
        self.edge_id = None             # ... and pooled edge -> parent edge, -1 for a padded one
        self.edge_src = None            # a dense-pooled batch (nn.diff_pool_static): pooled edge -> its entry of S^T A S, or -1
        self._degree_bound = None       # a dense-pooled batch and what is pooled from it: the most edges of a live row (K)
        self._node_bound = None         # ... and the most nodes of one graph (K; K_blk after nn.asap_static)
        self.node_score = None          # an ASAP-pooled batch (nn.asap_static): the raw float32 cluster scores [parent n_cap]
        self.asap_blocks = None         # ... and the blocks P [B K_blk, K_blk] of S^T A1 S its edges were read from (None: K_blk = 0)

    def max_degree(self):
        """A bound of the edges of a live row, in either direction: the store's largest in- / out-degree for a batch of the
        store's own graphs (host work, once per store), num_clusters once a dense pool has replaced them."""
        if self._degree_bound is not None:
            return int(self._degree_bound)
        return max(self._store._max_degrees())

    def max_graph_nodes(self):
        """A bound of the nodes of one graph of the batch, host numbers only: the store's largest graph for a collated or
        SAG-pooled batch, num_clusters after a dense pool, K_blk after nn.asap_static."""
        if self._node_bound is not None:
            return int(self._node_bound)
        return int(self._store._max_graph_nodes())

    def asap_pooled_capacities(self, k=None, ratio=None):
        """StaticBatchCapacities of this batch pooled by nn.asap_static(k= / ratio=): host arithmetic, no device.

        Graph g of n_g nodes keeps m_g = min(k, n_g) clusters, or min(n_g, int(ceilf(float32(n_g) * float32(ratio)))) — the
        rule of tfgx_segment_topk.  Both are non-decreasing in n_g (a float32 product by a non-negative constant, a ceiling and
        a minimum all are), so with n_max = max_graph_nodes() no graph keeps more than K_blk = rule(n_max) clusters; the float32
        product is evaluated as the kernel evaluates it (one rounding), not bounded.

            max_nodes = m_max of pooled_capacities(k / ratio)            (sum_g m_g <= m_max: DESIGN.md 2.27)
            max_edges = K_blk * m_max

        for the pooled graph of slot g is a subset of the m_g x m_g block, self-loops included, and
        sum_g m_g^2 <= (max_g m_g) * sum_g m_g <= K_blk * m_max.  The sink degree d stays; sinks = max(1, ceil(max_edges / d)).
        From one ASAP level to the next the edges shrink, as K_blk and m_max do; the first level's bound can exceed a sparse
        parent's max_edges.  K_blk itself is asap_clusters_per_graph.
        ValueError: what pooled_capacities refuses, sizes beyond int32."""
        cap = self.capacities
        m_max = int(self.pooled_capacities(k=k, ratio=ratio).max_nodes)            # validates k / ratio
        K_blk = self.asap_clusters_per_graph(k=k, ratio=ratio)
        B, d = int(cap.batch_size), int(cap.sink_degree)
        max_edges = K_blk * m_max
        sinks = max(1, -(-max_edges // d))
        if m_max + sinks >= (1 << 31) - 1 or max_edges >= (1 << 31) - 1:
            raise ValueError("asap_pooled_capacities: {} kept nodes + {} sinks, {} edges ({} clusters per graph at most) do not "
                             "fit int32".format(m_max, sinks, max_edges, K_blk))
        return type(cap)(B, m_max, max_edges, d, sinks, m_max + sinks, max_edges)

    def asap_clusters_per_graph(self, k=None, ratio=None):
        """K_blk: the most clusters nn.asap_static(k= / ratio=) keeps of one graph of this batch — the selection's rule applied
        to max_graph_nodes(), in float32 exactly as the kernel does.  Host arithmetic."""
        import math
        self.pooled_capacities(k=k, ratio=ratio)                                    # validates k / ratio
        n_max = self.max_graph_nodes()
        if k is not None:
            return min(int(k), n_max)
        return min(n_max, int(math.ceil(float(np.float32(n_max) * np.float32(ratio)))))

    def dense_pooled_capacities(self, num_clusters, drop_diagonal=False):
        """StaticBatchCapacities of this batch pooled by nn.diff_pool_static / nn.min_cut_pool_static (drop_diagonal=True) into
        K = num_clusters clusters per graph: host arithmetic, no device.  Every live slot becomes exactly K rows and at most
        K K edges (K (K - 1) without the diagonal), so max_nodes = B K and max_edges = B K K are reached by a batch of B live
        slots with dense blocks and exceeded by none; the sink degree d stays and sinks = max(1, ceil(max_edges / d)).
        ValueError: a K that is no integer of at least 1, sizes beyond int32."""
        cap = self.capacities
        K = num_clusters
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
            raise ValueError("dense_pooled_capacities: num_clusters must be an integer of at least 1, got {!r}".format(K))
        B, K, d = int(cap.batch_size), int(K), int(cap.sink_degree)
        max_nodes = B * K
        max_edges = B * K * (K - 1 if drop_diagonal else K)
        sinks = max(1, -(-max_edges // d))
        if max_nodes + sinks >= (1 << 31) - 1 or B * K * K >= (1 << 31) - 1:
            raise ValueError("dense_pooled_capacities: {} slots of {} clusters ({} rows + {} sinks, {} edges) do not fit "
                             "int32".format(B, K, max_nodes, sinks, max_edges))
        return type(cap)(B, max_nodes, max_edges, d, sinks, max_nodes + sinks, max_edges)

    def readout(self, h, op="mean"):
        """[B, F]: the `op` ("mean" / "sum" / "max" / "min") of h over the nodes of each slot, through the graph plan the batch
        carries (no sort, no host read).  The dead graph B is dropped, and the rows of dead slots are EXACTLY zero (torch.where
        on graph_mask): an empty graph's max is float32 lowest, which overflows in the next dense layer, and inf * 0 in a weight
        gradient is NaN."""
        from ..nn.pool import common_pool as P
        if op not in self._READOUTS:
            raise ValueError("readout: op must be one of {}, got {!r}".format(self._READOUTS, op))
        pooled = getattr(P, op + "_pool")(h, self.node_graph_index, self.num_graphs, cache=self.cache)[:self.num_slots]
        return torch.where(self.graph_mask[:, None], pooled, torch.zeros((), dtype=pooled.dtype, device=pooled.device))

    def to_3d(self, h, k):
        """[B, k, F]: utils.convert_x_to_3d of h ([n_cap, F]) over the slots — slot j of graph g is its j-th row, longer graphs
        are cut off, the rest and every dead slot is exactly zero.  One launch over graph_row_ptr (the dead graph B and the
        padded rows are never read), no host read."""
        from ..nn.pool.sort_pool_3d import rows_3d_static
        return rows_3d_static(h, self, k)

    def pooled_capacities(self, k=None, ratio=None):
        """StaticBatchCapacities of this batch pooled by nn.sag_pool_static(k= / ratio=): host arithmetic, no device.  The
        batch size, max_edges (kept edges are a subset of the live ones), the sink degree and the sinks P stay; max_nodes
        becomes m_max, a bound of the kept nodes sum_g k_g under the kernel's rule k_g = min(k, n_g), or
        min(n_g, int(ceilf(float32(n_g) * float32(ratio)))):

            k     : m_max = min(max_nodes, B * k)
            ratio : m_max = min(max_nodes, ceil(float32(ratio) * max_nodes * (1 + 2^-22)) + B)      (evaluated exactly)

        (each float32 product is at most the exact one times 1 + 2^-22, each ceil adds less than 1, there are at most B live
        graphs, and the live nodes are within max_nodes: DESIGN.md §2.27).  ValueError: both or neither of k / ratio, a
        negative or non-finite value, a k that is no integer, sizes beyond int32."""
        import fractions
        import math
        cap = self.capacities
        if (k is None) == (ratio is None):
            raise ValueError("pooled_capacities: give either k or ratio, {}".format(
                "not both of them" if k is not None else "got neither"))
        B = int(cap.batch_size)
        if k is not None:
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
                raise ValueError("pooled_capacities: k must be an integer of at least 0, got {!r}".format(k))
            if int(k) >= (1 << 31) - 1:
                raise ValueError("pooled_capacities: k = {} does not fit int32".format(k))
            m_max = min(int(cap.max_nodes), B * int(k))
        else:
            if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.integer, np.floating)):
                raise ValueError("pooled_capacities: ratio must be a number of at least 0, got {!r}".format(ratio))
            r32 = float(np.float32(ratio))
            if not (r32 >= 0.0) or math.isinf(r32):
                raise ValueError("pooled_capacities: ratio must be a finite number of at least 0, got {!r}".format(ratio))
            bound = fractions.Fraction(r32) * int(cap.max_nodes) * (1 + fractions.Fraction(1, 1 << 22))
            m_max = min(int(cap.max_nodes), math.ceil(bound) + B)
        if m_max + int(cap.sinks) >= (1 << 31) - 1:
            raise ValueError("pooled_capacities: {} kept nodes + {} sinks do not fit int32".format(m_max, cap.sinks))
        return type(cap)(B, m_max, cap.max_edges, cap.sink_degree, cap.sinks, m_max + cap.sinks, cap.e_cap)

    def check(self):
        """The ONE host read of a static batch, when the caller wants it: ValueError naming the first id outside [-1, G), or
        the first slot dropped because the batch would exceed max_nodes / max_edges.  Either slot is dead in this batch.  A
        pooled batch (nn.sag_pool_static) carries its parent's flags on, so it names the same slot; its own two flags — kept
        nodes beyond its capacities, a graph longer than the selection's cap — are named too."""
        B = self.num_slots
        host = torch.cat([self.counts[3:4].long(), self._given_ids.reshape(-1).long(), self.graph_mask.long()]).cpu().numpy()      # the one read
        flags, ids, mask = int(host[0]), host[1:1 + B], host[1 + B:] != 0
        if flags == 0:
            return self
        if flags & L.STATIC_POOL_TOO_LONG:
            raise ValueError("sag_pool_static: a graph of the batch has more than {} nodes (TFGX_STATIC_POOL_MAX_GRAPH_NODES) "
                             "and kept none".format(L.STATIC_POOL_MAX_GRAPH_NODES))
        if flags & L.STATIC_POOL_CLAMPED:
            raise ValueError("sag_pool_static: the kept nodes exceeded max_nodes = {} of the pooled capacities and were cut "
                             "off: the capacities were not made by pooled_capacities for this k / ratio".format(
                                 self.capacities.max_nodes))
        if flags & L.COLLATE_STATIC_BAD_ID:
            bad = np.nonzero((ids < -1) | (ids >= self._store_len))[0]
            raise ValueError("collate_static: graph id {} (slot {} of the batch) is outside [0, {}) and is not -1".format(
                int(ids[bad[0]]), int(bad[0]), self._store_len))
        dropped = np.nonzero((ids >= 0) & (ids < self._store_len) & ~mask)[0]
        raise ValueError("collate_static: slot {} (graph {}) and every later slot were dropped: the batch would exceed max_nodes "
                         "= {} or max_edges = {}".format(int(dropped[0]), int(ids[dropped[0]]), self.capacities.max_nodes,
                                                         self.capacities.max_edges))
