# coding=utf-8
"""Set2Set as a layer object (reference: tf_geometric/layers/pool/set2set.py)."""
from ...nn.pool.set2set import set2set
from ..rnn import LSTM
from .._base import Layer


class Set2Set(Layer):
    """inputs = [x, node_graph_index] or [x, node_graph_index, num_graphs] -> [num_graphs, 2F].  The trainable weights are
    those of self.lstm = LSTM(F, return_sequences=True, return_state=True), built for an input of width 2F (:22-26)."""

    def __init__(self, num_iterations=4, batch_graphs=False, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.num_iterations = num_iterations
        self.batch_graphs = batch_graphs
        self.lstm = None

    def build(self, input_shapes):
        f = int(input_shapes[0][-1])
        self.lstm = LSTM(f, return_sequences=True, return_state=True, seed=None if self._seed is None else int(self._seed) + 1)
        self.lstm.build([(1, 1, 2 * f)])
        self.lstm.built = True
        self.lstm.trainable(self._trainable)

    def trainable(self, flag=True):
        super().trainable(flag)
        if self.lstm is not None:
            self.lstm.trainable(flag)
        return self

    def parameters(self):
        return self.lstm.parameters() if self.lstm is not None else []

    @property
    def losses(self):
        return self.lstm.losses if self.lstm is not None else []

    def call(self, inputs, cache=None, training=None, mask=None):
        x, node_graph_index = inputs[0], inputs[1]
        num_graphs = inputs[2] if len(inputs) > 2 else None
        return set2set(x, node_graph_index, self.lstm, self.num_iterations, training=training, num_graphs=num_graphs,
                       batch_graphs=self.batch_graphs, cache=cache)
