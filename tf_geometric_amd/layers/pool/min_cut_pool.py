# coding=utf-8
"""MinCutPool as a layer object (reference: layers/pool/min_cut_pool.py).  inputs = [x, edge_index, edge_weight,
node_graph_index] -> [pooled_x, pooled_edge_index, pooled_edge_weight, pooled_node_graph_index]."""
from ...nn.pool.min_cut_pool import min_cut_pool
from ...nn.pool.dense_pool_static import min_cut_pool_static
from .diff_pool import DensePool


class MinCutPool(DensePool):
    """OOP API for MinCutPool: "Spectral Clustering with Graph Neural Networks for Graph Pooling"; constructor arguments as
    layers/pool/min_cut_pool.py:14-16.  The reference hands the loss callable of every call to keras (add_loss, :69); here
    the layer keeps the callable of its LATEST call and `losses` evaluates it after the regulariser terms."""

    def __init__(self, feature_gnn, assign_gnn, units, num_clusters, activation=None, use_bias=True,
                 gnn_use_normed_edge=True, bias_regularizer=None, *args, **kwargs):
        super().__init__(feature_gnn, assign_gnn, units, num_clusters, activation=activation, use_bias=use_bias,
                         bias_regularizer=bias_regularizer, *args, **kwargs)
        self.gnn_use_normed_edge = gnn_use_normed_edge
        self.loss_func = None

    @property
    def losses(self):
        """The base class's regulariser terms, then (cut_loss, orth_loss) of the latest call."""
        out = list(super().losses)
        if self.loss_func is not None:
            out.extend(self.loss_func())
        return out

    def call(self, inputs, cache=None, training=None, mask=None, return_loss_func=False, return_losses=False,
             num_graphs=None):
        if return_loss_func and return_losses:
            raise ValueError("return_loss_func and return_losses cannot be set to True at the same time")      # :58-59
        x, edge_index, edge_weight, node_graph_index = inputs
        outputs, loss_func = min_cut_pool(x, edge_index, edge_weight, node_graph_index, self.feature_gnn, self.assign_gnn,
                                          self.num_clusters, bias=self.bias, activation=self.activation,
                                          gnn_use_normed_edge=self.gnn_use_normed_edge, training=training, cache=cache,
                                          return_loss_func=True, num_graphs=num_graphs)
        self.loss_func = loss_func
        if return_loss_func:
            return outputs, loss_func
        if return_losses:
            return outputs, loss_func()
        return outputs

    def pool_static(self, x, batch, training=None, return_loss_func=False, return_losses=False):
        """The layer on a StaticBatchGraph: the pooled StaticBatchGraph of nn.min_cut_pool_static (with the loss callable or
        the two losses, means over the live slots, when asked for).  `losses` evaluates the latest call's.  No host read;
        capturable."""
        if return_loss_func and return_losses:
            raise ValueError("return_loss_func and return_losses cannot be set to True at the same time")
        pooled, loss_func = min_cut_pool_static(x, batch, self.feature_gnn, self.assign_gnn, self.num_clusters, bias=self.bias,
                                                activation=self.activation, gnn_use_normed_edge=self.gnn_use_normed_edge,
                                                return_loss_func=True, training=training)
        self.loss_func = loss_func
        if return_loss_func:
            return pooled, loss_func
        if return_losses:
            return pooled, loss_func()
        return pooled
