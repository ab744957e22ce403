# coding=utf-8
"""The link-prediction decoder: logit[e] = <z[row[e]], z_other[col[e]]> for an arbitrary, unsorted edge list.

The reference writes it inline (demo/demo_gae.py: two tf.gather and a reduce_sum, three [E, F] intermediates); here it is
one tfgx_edge_dot_f32 launch (include/tfgx_linkpred.h) that needs no plan.  When gradients are recorded the backward runs
on the aggregation kernels over the list's CSR plan (autograd._EdgeDot)."""
import torch

from ... import _lib as L
from ... import autograd as AG
from ...plan import CsrPlan, attach_plan, attached_plan


def _range_checked(edge_index, n_a, n_b):
    memo = getattr(edge_index, "_tfgx_edge_dot_range", None) if isinstance(edge_index, torch.Tensor) else None
    return memo is not None and memo[0] == edge_index._version and memo[1] <= n_a and memo[2] <= n_b


def edge_dot(z, edge_index, z_other=None, cache=None):
    """
    :param z: [n_a, F] node embeddings (rows are picked by edge_index[0])
    :param edge_index: [2, E], any order, duplicates and self-pairs allowed
    :param z_other: None: both endpoints read `z`; else [n_b, F], rows picked by edge_index[1]
    :param cache: only used when gradients are recorded: the dict that holds (or receives) the CSR plan of THIS edge list
        (CsrPlan.from_cache: cache, then edge_index._tfgx_plan, then one build that is memoised on the tensor)
    :return: float32 tensor [E]

    An endpoint outside its table raises TfgxError (code 2); the range flag is read from the device once per edge_index
    tensor (memoised on it), so repeat calls on the same list do not synchronise.
    """
    L.require_gpu()
    a = L.as_f32(z)
    b = a if z_other is None else L.as_f32(z_other, a.device)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("edge_dot: z and z_other must be [n, F] with the same F")
    ei = L.as_i32(edge_index, a.device)
    if ei.numel() == 0:
        ei = ei.reshape(2, 0)
    if ei.dim() != 2 or ei.shape[0] != 2:
        raise ValueError("edge_index must have shape [2, num_edges]")
    n_a, n_b, E = int(a.shape[0]), int(b.shape[0]), int(ei.shape[1])
    row, col = ei[0].contiguous(), ei[1].contiguous()
    if AG.needs_grad(a, b) and E > 0:
        plan = CsrPlan.from_cache(edge_index if isinstance(edge_index, torch.Tensor) else ei, n_a, n_b, cache)   # validates the endpoints
        if plan.num_edges != E or plan.n_dst != n_a or plan.n_src != n_b:
            raise ValueError("edge_dot: the plan found in cache / on edge_index describes a [{}, {}] operator with {} edges, "
                             "this call needs [{}, {}] with {}".format(plan.n_dst, plan.n_src, plan.num_edges, n_a, n_b, E))
        if cache is None and isinstance(edge_index, torch.Tensor) and attached_plan(edge_index) is None:
            attach_plan(edge_index, plan)
        return AG.edge_dot(plan, a, None if z_other is None else b, row, col)
    if _range_checked(edge_index, n_a, n_b):
        return AG.edge_dot_forward(a.detach(), b.detach(), row, col)
    flag = torch.zeros(1, dtype=torch.int32, device=a.device)
    out = AG.edge_dot_forward(a.detach(), b.detach(), row, col, bad_flag=flag)
    if int(flag.item()) != 0:
        raise L.TfgxError("tfgx_edge_dot_f32 failed with code 2: edge endpoint outside [0, {}) x [0, {})".format(n_a, n_b))
    if isinstance(edge_index, torch.Tensor):
        edge_index._tfgx_edge_dot_range = (edge_index._version, n_a, n_b)
    return out
