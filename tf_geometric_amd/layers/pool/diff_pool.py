# coding=utf-8
"""DiffPool as a layer object (reference: layers/pool/diff_pool.py).  inputs = [x, edge_index, edge_weight, node_graph_index]
-> [pooled_x, pooled_edge_index, pooled_edge_weight, pooled_node_graph_index]."""
from ...nn.pool.diff_pool import diff_pool
from ...nn.pool.dense_pool_static import diff_pool_static
from .._base import Layer


class DensePool(Layer):
    """What DiffPool and MinCutPool share: two GNNs, the number of clusters per graph and a `units`-sized zero-initialised
    bias, created in __init__ (the layer never sees the width of feature_gnn's output, so there is no lazy build).
    use_bias=False gives bias = None (the reference reads an unset attribute there).  parameters() and trainable() also
    reach the weights of the two GNNs when they are layers of this package."""

    def __init__(self, feature_gnn, assign_gnn, units, num_clusters, activation=None, use_bias=True, bias_regularizer=None,
                 *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.feature_gnn = feature_gnn
        self.assign_gnn = assign_gnn
        self.num_clusters = num_clusters
        self.activation = activation
        self.bias_regularizer = bias_regularizer
        if use_bias and units is None:
            raise Exception("The \"units\" parameter is required when you set use_bias=True.")          # diff_pool.py:36-37
        self.bias = self.add_weight("bias", [units], initializer="zeros") if use_bias else None
        self.built = True

    def build(self, input_shapes):
        """The bias is created in __init__."""

    def _gnns(self):
        seen = []
        for gnn in (self.feature_gnn, self.assign_gnn):
            if isinstance(gnn, Layer) and not any(gnn is s for s in seen):
                seen.append(gnn)
        return seen

    def parameters(self):
        """The bias and the weights the two GNNs hold at this moment (a GNN builds its weights on its first call)."""
        out = super().parameters()
        for gnn in self._gnns():
            out.extend(gnn.parameters())
        return out

    def trainable(self, flag=True):
        super().trainable(flag)
        for gnn in self._gnns():
            gnn.trainable(flag)
        return self


class DiffPool(DensePool):
    """OOP API for DiffPool: "Hierarchical graph representation learning with differentiable pooling"; constructor
    arguments as layers/pool/diff_pool.py:14-15."""

    def call(self, inputs, cache=None, training=None, mask=None, num_graphs=None):
        x, edge_index, edge_weight, node_graph_index = inputs
        return diff_pool(x, edge_index, edge_weight, node_graph_index, self.feature_gnn, self.assign_gnn, self.num_clusters,
                         bias=self.bias, activation=self.activation, training=training, cache=cache, num_graphs=num_graphs)

    def pool_static(self, x, batch, training=None):
        """The layer on a StaticBatchGraph (GraphStore.collate_static's, or an earlier pool_static's): the pooled
        StaticBatchGraph of nn.diff_pool_static with this layer's GNNs, clusters, bias and activation.  No host read;
        capturable."""
        return diff_pool_static(x, batch, self.feature_gnn, self.assign_gnn, self.num_clusters, bias=self.bias,
                                activation=self.activation, training=training)
