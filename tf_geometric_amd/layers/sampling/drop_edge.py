# coding=utf-8
"""DropEdge layer — drop-in for tf_geometric.layers.DropEdge (reference: layers/sampling/drop_edge.py)."""
from ...nn.sampling.drop_edge import drop_edge


class DropEdge(object):
    """DropEdge: Towards Deep Graph Convolutional Networks on Node Classification
    (https://openreview.net/forum?id=Hkx1qkrKPr).  Owns no weights.

    :param rate: dropout rate
    :param force_undirected: If set to `True`, will either drop or keep both edges of an undirected edge.
    """

    def __init__(self, rate=0.5, force_undirected=False):
        self.rate = rate
        self.force_undirected = force_undirected
        if self.rate < 0. or self.rate > 1.:                                                       # :21-23
            raise ValueError("Dropout probability has to be between 0 and 1, but got {}".format(self.rate))

    def parameters(self):
        return []

    def call(self, inputs, training=None, mask=None, seed=None, cache=None):
        """inputs = [edge_index, edge_attr, ...] -> the dropped list; `seed` / `cache` as nn.drop_edge."""
        return drop_edge(inputs=inputs, rate=self.rate, force_undirected=self.force_undirected, training=training,
                         seed=seed, cache=cache)

    def __call__(self, inputs, **kwargs):
        return self.call(inputs, **kwargs)
