# coding=utf-8
"""LSTM weights with Keras's names, shapes and default initialisers (tf.keras.layers.LSTM: kernel [F, 4 units],
recurrent_kernel [units, 4 units], bias [4 units], gate order i, f, c, o).  Called on a dense [B, T, F] tensor it runs the
recurrence on the sequence kernel of include/tfgx_set2set.h; handed to nn.lstm_graph_sage it is a weight holder and that
layer's own kernel runs the recurrence."""
import math

import torch

from .. import _lib as L
from ._base import Layer


class LSTM(Layer):
    def __init__(self, units, kernel_regularizer=None, bias_regularizer=None, unit_forget_bias=True, return_sequences=False,
                 return_state=False, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.units = int(units)
        self.return_sequences = bool(return_sequences)
        self.return_state = bool(return_state)
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

    def __call__(self, inputs, **kwargs):
        """`inputs` is ONE dense tensor [B, T, F] (Keras's call shape), not a list."""
        self._maybe_build([inputs])
        return self.call(inputs, **kwargs)

    def call(self, inputs, initial_state=None, training=None, mask=None):
        """tf.keras.layers.LSTM on a dense [B, T, F] tensor.  initial_state = [h0, c0], each [B, units] or [1, units]
        (broadcast over the batch); None: zeros.  Returns the last h [B, units], or every h_t [B, T, units] with
        return_sequences; with return_state that followed by the last h and the last c.  `training` changes nothing (no
        dropout is configured).  The input projection is one GEMM over [B * T, F]; tfgx_lstm_sequence_f32 owns the
        recurrence.  Units that are no multiple of 16 are zero-padded to the next one, which is exact (a padded unit
        stays at h = c = 0).  Differentiable in the input, kernel, recurrent_kernel, bias, h0 and c0."""
        from .. import autograd as AG
        from ..nn.conv.graph_sage import _pad_gate_blocks
        from ..plan import gemm_bias_act
        x = L.as_f32(inputs)
        if x.dim() != 3:
            raise ValueError("LSTM: the input must be [batch, steps, features], got shape {}".format(tuple(x.shape)))
        B, T, F = (int(v) for v in x.shape)
        U = self.units
        if int(self.kernel.shape[0]) != F:
            raise ValueError("LSTM: built for {} input features, got {}".format(int(self.kernel.shape[0]), F))
        Up = (U + 15) // 16 * 16
        if Up > L.LSTM_MAX_UNITS:
            raise ValueError("LSTM: {} units (padded to {}) exceed TFGX_LSTM_MAX_UNITS = {}".format(U, Up, L.LSTM_MAX_UNITS))
        state = []
        for k in range(2):
            s = None if initial_state is None else L.as_f32(initial_state[k])
            if s is None:
                s = torch.zeros((B, Up), dtype=torch.float32, device=x.device)
            else:
                if s.dim() != 2 or int(s.shape[1]) != U or int(s.shape[0]) not in (1, B):
                    raise ValueError("LSTM: initial_state[{}] must be [{} or 1, {}], got {}".format(k, B, U, tuple(s.shape)))
                s = torch.nn.functional.pad(s.expand(B, U), (0, Up - U)) if Up != U else s.expand(B, U)
            state.append(s)
        if B == 0 or T == 0:
            seq, h, c = x.new_zeros((B, T, U)), state[0][:, :U], state[1][:, :U]
        else:
            kp, bp = _pad_gate_blocks(L.as_f32(self.kernel), U, Up), _pad_gate_blocks(L.as_f32(self.bias), U, Up)
            rp = _pad_gate_blocks(L.as_f32(self.recurrent_kernel), U, Up)
            if Up != U:
                rp = torch.nn.functional.pad(rp, (0, 0, 0, Up - U))
            x2 = x.reshape(B * T, F)
            P = AG.linear(x2, kp, bp) if AG.needs_grad(x2, kp, bp) else gemm_bias_act(x2, kp, bias=bp.contiguous())
            seq, h, c = AG.lstm_sequence(P, B, T, rp, state[0], state[1])
            seq = seq.reshape(B, T, Up)
            if Up != U:
                seq, h, c = seq[:, :, :U], h[:, :U], c[:, :U]
        out = seq if self.return_sequences else h
        return [out, h, c] if self.return_state else out
