# coding=utf-8
"""Set2Set readout (reference: tf_geometric/nn/pool/set2set.py:8-42): num_iterations rounds of an LSTM over the per-graph
query and an attention readout of the nodes under it.  Per round one LSTM launch (tfgx_lstm_sequence_f32) and one attention
launch (tfgx_set2set_attend_f32: online softmax, x read once, only [G, F] written) — DESIGN.md §2.16."""
import torch

from ... import _lib as L
from ... import autograd as AG
from .common_pool import CACHE_KEY_GRAPH_PLAN, _graph_plan          # noqa: F401 - shared with the dense pooling layers


def set2set(x, node_graph_index, lstm, num_iterations, training=None, num_graphs=None, batch_graphs=False, cache=None):
    """[num_graphs, 2F] graph features.

    `lstm`: any callable with the Keras call shape of set2set.py:31 — lstm(seq [B, T, 2F], initial_state=[h, c],
    training=...) -> (sequence [B, T, F], h [B, F], c [B, F]); layers.LSTM(F, return_sequences=True, return_state=True) runs
    on the sequence kernel.
    batch_graphs=False reproduces the reference literally: the query tensor goes in as h[None], ONE sequence whose steps are
    the graphs of the batch, with a [1, F] state carried from the last graph of a round to the first graph of the next — so
    a graph's output depends on the graphs before it.  batch_graphs=True runs h[:, None] with a [G, F] state: G sequences
    of one step, every graph independent of its batch (the form of the paper).
    num_graphs=None reads max(node_graph_index) + 1 from the device as the reference does (one host synchronisation);
    passing it avoids that one.  Building the graph plan synchronises once more (the plan builder reports bad indices to the
    host), so a call is free of host synchronisation only with num_graphs given AND a `cache` that already holds the plan:
    pass the int32 device tensor of graph ids itself (a converted copy is a new tensor and rebuilds the plan)."""
    x = L.as_f32(x)
    ids = L.as_i32(node_graph_index, x.device).reshape(-1)
    if x.dim() != 2 or int(ids.shape[0]) != int(x.shape[0]):
        raise ValueError("set2set: x must be [num_nodes, F] with one graph index per node, got {} and {}".format(
            tuple(x.shape), tuple(ids.shape)))
    n, F = int(x.shape[0]), int(x.shape[1])
    if F > L.LSTM_MAX_UNITS:
        raise ValueError("set2set: {} features need an LSTM of {} units, above TFGX_LSTM_MAX_UNITS = {}".format(
            F, F, L.LSTM_MAX_UNITS))
    if num_graphs is None:
        if n == 0:
            raise ValueError("set2set: num_graphs cannot be derived from an empty node_graph_index")
        num_graphs = int(ids.max().item()) + 1                          # set2set.py:21
    G = int(num_graphs)
    plan = _graph_plan(ids, G, n, cache)
    h = torch.zeros((G, 2 * F), dtype=torch.float32, device=x.device)      # :25
    rows = G if batch_graphs else 1
    state = [torch.zeros((rows, F), dtype=torch.float32, device=x.device) for _ in range(2)]      # :26
    if G == 0:
        return h
    for _ in range(int(num_iterations)):
        seq = h.unsqueeze(1) if batch_graphs else h.unsqueeze(0)        # :30
        out, state_h, state_c = lstm(seq, initial_state=state, training=training)
        state = [state_h, state_c]
        q = L.as_f32(out).reshape(G, -1)                                # :33
        if int(q.shape[1]) != F:
            raise ValueError("set2set: the lstm must return {} units per step (the feature width), got {}".format(
                F, int(q.shape[1])))
        r = AG.set2set_attend(plan, x, q)                               # :35-39 in one launch
        h = torch.cat([q, r], dim=-1)                                   # :40
    return h
