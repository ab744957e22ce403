# coding=utf-8
"""Graph-level readouts as segment reduces over node_graph_index — the same kernel as the
neighbour aggregation, with "destination" = graph id.  Reference: tf_geometric/nn/pool/common_pool.py:7-52."""
import torch

from ... import _lib as L
from ...plan import CsrPlan, segment_reduce
from ... import autograd as AG


def _pool(x, node_graph_index, num_graphs, op, cache=None):
    x = L.as_f32(x)
    ids = L.as_i32(node_graph_index)
    if num_graphs is None:
        num_graphs = int(ids.max().item()) + 1                      # :8-9
    n = int(ids.shape[0])
    if cache is not None:
        # the graph plan a batch carries (GraphStore.collate / collate_static leave it in batch.cache): no sort, no host read
        plan = _graph_plan(ids, int(num_graphs), n, cache)
    else:
        plan = CsrPlan.build(torch.stack([ids, torch.arange(n, dtype=torch.int32, device=ids.device)]), int(num_graphs),
                             max(n, 1))
    if AG.needs_grad(x):         # graph classification trains THROUGH the readout (the reference's TF ops all have gradients)
        return plan, x, AG.aggregate(plan, x, op)
    return plan, x, segment_reduce(plan, x, op)


def sum_pool(x, node_graph_index, num_graphs=None, cache=None):
    """:17-21.  `cache` (here and in the three readouts below): the batch's cache dict — the graph plan is taken from it
    (and kept there when it has to be built), as _graph_plan describes; without one the plan is built on every call."""
    return _pool(x, node_graph_index, num_graphs, L.SUM, cache)[2]


def mean_pool(x, node_graph_index, num_graphs=None, cache=None):
    """sum / (count + 1e-8) — note the epsilon form, not max(count, 1) (:7-12)."""
    plan, _, s = _pool(x, node_graph_index, num_graphs, L.SUM, cache)
    return s / (plan.in_degree().to(torch.float32).unsqueeze(-1) + 1e-8)


def max_pool(x, node_graph_index, num_graphs=None, cache=None):
    """unsorted_segment_max; an empty graph holds float32 lowest (:41-45)."""
    return _pool(x, node_graph_index, num_graphs, L.MAX, cache)[2]


def min_pool(x, node_graph_index, num_graphs=None, cache=None):
    """unsorted_segment_min = -max(-x); an empty graph holds float32 max (:48-52)."""
    x = L.as_f32(x)
    return -_pool(-x, node_graph_index, num_graphs, L.MAX, cache)[2]


CACHE_KEY_GRAPH_PLAN = "tfgx_set2set_graph_plan"


def _graph_plan(ids, num_graphs, n, cache):
    """The CSR over graphs (rows = graphs, col = node ids in stable order): built once per call.  With a `cache` it is kept
    there together with the ids tensor it was built from (kept alive, so its address stays its own) and reused only for that
    very storage, unmodified (same address, shape and version counter) and the same num_graphs; anything else rebuilds it.  Building synchronises once
    (tfgx_build_csr_by_dst reports bad indices to the host)."""
    hit = None if cache is None else cache.get(CACHE_KEY_GRAPH_PLAN)
    if hit is not None and hit[0].data_ptr() == ids.data_ptr() and hit[0].shape == ids.shape and hit[1] == ids._version \
            and hit[2].n_dst == num_graphs:
        return hit[2]
    plan = CsrPlan.build(torch.stack([ids, torch.arange(n, dtype=torch.int32, device=ids.device)]), num_graphs, max(n, 1))
    if cache is not None:
        cache[CACHE_KEY_GRAPH_PLAN] = (ids, ids._version, plan)
    return plan
