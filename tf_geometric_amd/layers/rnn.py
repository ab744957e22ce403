# coding=utf-8
"""LSTM weights with Keras's names, shapes and default initialisers (tf.keras.layers.LSTM: kernel [F, 4 units],
recurrent_kernel [units, 4 units], bias [4 units], gate order i, f, c, o).  A weight holder: the recurrence itself runs inside
the layers that take one (nn.lstm_graph_sage)."""
import math

import torch

from .. import _lib as L
from ._base import Layer


class LSTM(Layer):
    def __init__(self, units, kernel_regularizer=None, bias_regularizer=None, unit_forget_bias=True, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.units = int(units)
        self.kernel_regularizer = kernel_regularizer
        self.bias_regularizer = bias_regularizer
        self.unit_forget_bias = unit_forget_bias
        self.kernel = None
        self.recurrent_kernel = None
        self.bias = None

    def build(self, input_shape):
        f, u = int(input_shape[0][-1]), self.units
        dev = L.device()
        self.kernel = self.add_weight("kernel", [f, 4 * u], "glorot_uniform")
        # Keras's orthogonal initialiser: Q of a normal [4u, u] matrix, signs fixed by R's diagonal, transposed to [u, 4u]
        a = torch.randn((4 * u, u), generator=self._rng(dev), dtype=torch.float64)
        q, r = torch.linalg.qr(a)
        q = q * torch.sign(torch.diagonal(r)).unsqueeze(0)
        self.recurrent_kernel = q.t().contiguous().to(torch.float32).to(dev)
        self._weights["recurrent_kernel"] = self.recurrent_kernel
        self._init_of["recurrent_kernel"] = "orthogonal"
        self.bias = self.add_weight("bias", [4 * u], "zeros")
        if self.unit_forget_bias:
            self.bias[u:2 * u] = 1.0

    @property
    def losses(self):
        """Keras regularises kernel and bias here; the recurrent kernel has its own (unset) regulariser."""
        out = []
        if self.kernel_regularizer is not None and self.kernel is not None:
            out.append(self.kernel_regularizer(self.kernel))
        if self.bias_regularizer is not None and self.bias is not None:
            out.append(self.bias_regularizer(self.bias))
        return out

    def call(self, inputs, **kwargs):
        raise NotImplementedError("layers.LSTM holds weights; pass it to nn.lstm_graph_sage / layers.LSTMGraphSage")
