# coding=utf-8
"""ASAP as a layer object (reference: layers/pool/asap.py).  inputs = [x, edge_index, edge_weight, node_graph_index] ->
[pooled_x, pooled_edge_index, pooled_edge_weight, pooled_node_graph_index]."""
import torch

from ...nn.pool.asap import asap
from ...nn.pool.asap_static import asap_static
from .._base import Layer


class ASAP(Layer):
    """The eleven weights carry the reference's names and initialisers (layers/pool/asap.py:50-87).  The LEConv kernels are
    [num_features, 1]: LEConv scores the CLUSTER features, which are as wide as x (nn/pool/asap.py:79-91).  The reference
    registers them as [attention_units, 1], which only runs when attention_units == num_features; here any attention_units
    works."""

    def __init__(self, k=None, ratio=None, drop_rate=0.0, attention_units=None, le_conv_activation=torch.sigmoid,
                 le_conv_use_bias=True, kernel_regularizer=None, bias_regularizer=None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.attention_units = attention_units
        self.attention_gcn_kernel = None
        self.attention_gcn_bias = None
        self.attention_query_kernel = None
        self.attention_query_bias = None
        self.attention_score_kernel = None
        self.attention_score_bias = None
        self.le_conv_self_kernel = None
        self.le_conv_self_bias = None
        self.le_conv_aggr_self_kernel = None
        self.le_conv_aggr_self_bias = None
        self.le_conv_aggr_neighbor_kernel = None
        self.k = k
        self.ratio = ratio
        self.drop_rate = drop_rate
        self.le_conv_activation = le_conv_activation
        self.le_conv_use_bias = le_conv_use_bias
        self.kernel_regularizer = kernel_regularizer
        self.bias_regularizer = bias_regularizer

    def build(self, input_shapes):
        num_features = int(input_shapes[0][-1])
        if self.attention_units is None:
            self.attention_units = num_features
        a = int(self.attention_units)
        self.attention_gcn_kernel = self.add_weight("attention_gcn_kernel", [num_features, a])
        self.attention_gcn_bias = self.add_weight("attention_gcn_bias", [a], initializer="zeros")
        self.attention_query_kernel = self.add_weight("attention_query_kernel", [a, a])
        self.attention_query_bias = self.add_weight("attention_query_bias", [a], initializer="zeros")
        self.attention_score_kernel = self.add_weight("attention_score_kernel", [2 * a, 1])
        self.attention_score_bias = self.add_weight("attention_score_bias", [1], initializer="zeros")
        self.le_conv_self_kernel = self.add_weight("le_conv_self_kernel", [num_features, 1])
        if self.le_conv_use_bias:
            self.le_conv_self_bias = self.add_weight("le_conv_self_bias", [1], initializer="zeros")
        self.le_conv_aggr_self_kernel = self.add_weight("le_conv_aggr_self_kernel", [num_features, 1])
        if self.le_conv_use_bias:
            self.le_conv_aggr_self_bias = self.add_weight("le_conv_aggr_self_bias", [1], initializer="zeros")
        self.le_conv_aggr_neighbor_kernel = self.add_weight("le_conv_aggr_neighbor_kernel", [num_features, 1])

    def call(self, inputs, cache=None, training=None, mask=None, seed=None):
        x, edge_index, edge_weight, node_graph_index = inputs
        return asap(x, edge_index, edge_weight, node_graph_index,
                    self.attention_gcn_kernel, self.attention_gcn_bias,
                    self.attention_query_kernel, self.attention_query_bias,
                    self.attention_score_kernel, self.attention_score_bias,
                    self.le_conv_self_kernel, self.le_conv_self_bias,
                    self.le_conv_aggr_self_kernel, self.le_conv_aggr_self_bias,
                    self.le_conv_aggr_neighbor_kernel, None,
                    k=self.k, ratio=self.ratio, le_conv_activation=self.le_conv_activation,
                    drop_rate=self.drop_rate, training=training, cache=cache, seed=seed)

    def pool_static(self, x, batch, training=None, seed=None):
        """The layer on a StaticBatchGraph (GraphStore.collate_static's, or an earlier pool_static's): the pooled
        StaticBatchGraph of nn.asap_static with this layer's weights (built on first use, as call builds them), k / ratio,
        activation and drop_rate.  No host read; capturable."""
        self._maybe_build([x])
        return asap_static(x, batch,
                           self.attention_gcn_kernel, self.attention_gcn_bias,
                           self.attention_query_kernel, self.attention_query_bias,
                           self.attention_score_kernel, self.attention_score_bias,
                           self.le_conv_self_kernel, self.le_conv_self_bias,
                           self.le_conv_aggr_self_kernel, self.le_conv_aggr_self_bias,
                           self.le_conv_aggr_neighbor_kernel,
                           k=self.k, ratio=self.ratio, le_conv_activation=self.le_conv_activation,
                           drop_rate=self.drop_rate, training=training, seed=seed)
