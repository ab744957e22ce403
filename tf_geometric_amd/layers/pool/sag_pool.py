# coding=utf-8
"""SAGPool / SortPool as layer objects (reference: layers/pool/sag_pool.py, layers/pool/sort_pool.py).
inputs = [x, edge_index, edge_weight, node_graph_index] -> [pooled_x, pooled_edge_index, pooled_edge_weight,
pooled_node_graph_index]."""
from ...nn.pool.sag_pool import sag_pool
from ...nn.pool.sag_pool_static import sag_pool_static
from ...nn.pool.sort_pool import sort_pool
from ...nn.pool.sort_pool_3d import sort_pool_3d, sort_pool_static
from .._base import Layer


class SAGPool(Layer):
    """The trainable weights are the score GNN's: parameters() and trainable() forward to it."""

    def __init__(self, score_gnn, k=None, ratio=None, score_activation=None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.score_gnn = score_gnn
        self.k = k
        self.ratio = ratio
        self.score_activation = score_activation

    def build(self, input_shapes):
        """SAGPool owns no weights of its own."""

    def parameters(self):
        return list(self.score_gnn.parameters())

    def trainable(self, flag=True):
        self._trainable = bool(flag)
        self.score_gnn.trainable(flag)
        return self

    def call(self, inputs, cache=None, training=None, mask=None):
        x, edge_index, edge_weight, node_graph_index = inputs
        return sag_pool(x, edge_index, edge_weight, node_graph_index, self.score_gnn, k=self.k, ratio=self.ratio,
                        score_activation=self.score_activation, training=training, cache=cache)

    def pool_static(self, x, batch, training=None, capacities=None):
        """The layer on a StaticBatchGraph (GraphStore.collate_static's, or an earlier pool_static's): the pooled
        StaticBatchGraph of nn.sag_pool_static with this layer's k / ratio / activation.  No host read; capturable."""
        return sag_pool_static(x, batch, self.score_gnn, k=self.k, ratio=self.ratio, score_activation=self.score_activation,
                               training=training, capacities=capacities)


class SortPool(Layer):
    def __init__(self, k=None, ratio=None, sort_index=-1, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.k = k
        self.ratio = ratio
        self.sort_index = sort_index

    def build(self, input_shapes):
        """SortPool owns no weights."""

    def call(self, inputs, training=None, mask=None):
        x, edge_index, edge_weight, node_graph_index = inputs
        return sort_pool(x, edge_index, edge_weight, node_graph_index, k=self.k, ratio=self.ratio,
                         sort_index=self.sort_index, training=training)

    def pool_3d(self, inputs, num_graphs=None, cache=None):
        """The DGCNN readout of this layer's k and sort_index: nn.sort_pool_3d, [num_graphs, k, F] in one launch, no pooled
        edge list.  inputs = [x, node_graph_index], or the 4-list call() takes (its edges are not looked at)."""
        if len(inputs) == 2:
            x, node_graph_index = inputs
        else:
            x, _, _, node_graph_index = inputs
        return sort_pool_3d(x, node_graph_index, k=self.k, sort_index=self.sort_index, num_graphs=num_graphs, cache=cache,
                            ratio=self.ratio)

    def pool_static(self, x, batch):
        """The same readout on a StaticBatchGraph (nn.sort_pool_static): [B, k, F], no host read; capturable."""
        if self.ratio is not None:
            raise ValueError("SortPool.pool_static: ratio= has no 3-D form: construct the layer with k")
        return sort_pool_static(x, batch, self.k, sort_index=self.sort_index)
