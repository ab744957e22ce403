# coding=utf-8
"""DropEdge on the device — functional mirror of tf_geometric/nn/sampling/drop_edge.py.

Kernels: tfgx_drop_edge_count / tfgx_drop_edge_emit (include/tfgx_dropedge.h).  Edge e of the input list survives iff
tfgx_dropout_keep(seed, e, rate): a counter-based rule the host can restate, so a call is reproduced by its seed.  One
host sync per call (the kept count); the rest is asynchronous.

A DropEdge training step draws a new edge list every step.  When the input edge list has a CSR plan (attached as
``edge_index._tfgx_plan`` by a producer, or held in ``cache``), the dropped list's plan — and, when the parent's
transposed plan exists, the transposed plan the backward pass needs — is derived from it by order-stable compactions
and handed on as ``dropped_edge_index._tfgx_plan`` (picked up by CsrPlan.from_cache and SparseMatrix.plan): the layers
after it do not sort.  DERIVE_PLANS is the dispatch rule."""
import ctypes

import numpy as np
import torch

from ... import _lib as L
from ...plan import CsrPlan, CACHE_KEY_PLAN, attach_plan, attached_plan
from ...utils.subgraph import refuse_capture

# Dispatch between deriving the dropped list's plans from the parent's (True) and sorting the dropped list again
# (CsrPlan.build, False), for an input of E edges.  NOT MEASURED yet (DESIGN.md §2.13 says why and what the estimate is):
# until tools/bench_drop_edge.py has run, derive whenever a parent plan exists; replace by a size threshold if its sweep
# puts the sort ahead anywhere.
def DERIVE_PLANS(num_edges):     # noqa: N802 - a policy constant that happens to be a function
    return True


_NO_NODE_COUNT = (1 << 31) - 2      # without a plan the node count is unknown: only negative endpoints are refused


def _seed_from_torch():
    """A fresh 64-bit seed from torch's default (CPU) generator: torch.manual_seed reproduces a run; no device work."""
    hi, lo = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
    return (hi << 32) | lo


def _parent_plan(edge_index, num_edges, cache):
    plan = attached_plan(edge_index, num_edges)
    if plan is None and cache is not None:
        plan = cache.get(CACHE_KEY_PLAN, None)
    if plan is not None and plan.num_edges != num_edges:
        plan = None          # a plan of another edge list: ignore it, never guess
    return plan


def _plan_io(parent, n_out, dev):
    io = L.DropEdgePlan()
    row_ptr = torch.empty(parent.n_dst + 1, dtype=torch.int32, device=dev)
    col = torch.empty(n_out, dtype=torch.int32, device=dev)
    perm = torch.empty(n_out, dtype=torch.int32, device=dev)
    io.parent_row_ptr, io.parent_col, io.parent_perm = parent.row_ptr.data_ptr(), parent.col.data_ptr(), parent.perm.data_ptr()
    io.out_row_ptr, io.out_col, io.out_perm = row_ptr.data_ptr(), col.data_ptr(), perm.data_ptr()
    return io, CsrPlan(row_ptr, col, perm, parent.n_dst, parent.n_src, n_out)


def drop_edge_index(edge_index, rate, seed, force_undirected=False, parent=None, derive=None):
    """The kernel call: (dropped edge_index [2, E'], edge_id [E'] original ids, plan or None) for a device int32
    edge_index.  `parent`: CsrPlan of edge_index or None; `derive`: None = DERIVE_PLANS, True / False = force."""
    lib = L.require_gpu()
    ei = L.as_i32(edge_index)
    if ei.numel() == 0:
        ei = ei.reshape(2, 0)
    if ei.dim() != 2 or ei.shape[0] != 2:
        raise ValueError("edge_index must have shape [2, num_edges]")
    E, dev = int(ei.shape[1]), ei.device
    if force_undirected:
        parent = None            # no derived plan for the mirrored form (the output is not a sub-list of the input)
    parent_t = parent._transposed if parent is not None else None
    if derive is None:
        derive = DERIVE_PLANS(E)
    derived = parent is not None and derive
    n_dst, n_src = (parent.n_dst, parent.n_src) if parent is not None else (_NO_NODE_COUNT, _NO_NODE_COUNT)
    row, col = ei[0].contiguous(), ei[1].contiguous()
    ws_bytes = lib.tfgx_drop_edge_workspace_bytes(E, n_dst, n_src, int(derived), int(derived and parent_t is not None))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    n_out = ctypes.c_int64(0)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    und = int(bool(force_undirected))
    L.check(lib.tfgx_drop_edge_count(L.ptr(row), L.ptr(col), E, n_dst, n_src, float(rate), seed, und, ctypes.byref(n_out),
                                     L.ptr(ws), ws_bytes, L.stream_ptr()), "tfgx_drop_edge_count")
    K = int(n_out.value)
    out = torch.empty((2, K), dtype=torch.int32, device=dev)
    edge_id = torch.empty(K, dtype=torch.int32, device=dev)
    io = io_t = plan = plan_t = None
    if derived:
        io, plan = _plan_io(parent, K, dev)
        if parent_t is not None:
            io_t, plan_t = _plan_io(parent_t, K, dev)
    L.check(lib.tfgx_drop_edge_emit(L.ptr(row), L.ptr(col), E, n_dst, n_src, float(rate), seed, und, K, L.ptr(out[0]),
                                    L.ptr(out[1]), L.ptr(edge_id), None if io is None else ctypes.byref(io),
                                    None if io_t is None else ctypes.byref(io_t), L.ptr(ws), ws_bytes, L.stream_ptr()),
            "tfgx_drop_edge_emit")
    if parent is not None and not derived:      # the rule put the sort ahead: still hand the plan on
        plan = CsrPlan.build(out, parent.n_dst, parent.n_src)
        if parent_t is not None:
            plan.transposed()
    elif plan is not None:
        plan._edge_index = out
        if plan_t is not None:
            plan_t._transposed = plan       # the flip of the flip: never rebuilt, the flipped list is never materialised
            plan._transposed = plan_t
    return out, edge_id, plan


def _gather_last_axis(attr, ids, mirrored):
    """attr[..., ids] (then repeated once more along the last axis for the mirrored form, whose ids are [ids | ids])."""
    if not isinstance(attr, torch.Tensor):
        out = np.take(attr, ids.cpu().numpy(), axis=-1)                       # reference :47
        return np.concatenate([out, out], axis=-1) if mirrored else out
    from ... import autograd as AG
    from ...utils.subgraph import gather_i32
    if attr.device != ids.device:
        attr = attr.to(ids.device)
    if attr.dtype == torch.float32 and attr.dim() >= 1:
        # rows of the flattened [d, E] attribute through the gather kernel; a tracked attribute gets a backward that is a
        # plain scatter into zeros (kept ids are unique)
        flat = attr.reshape(int(np.prod(attr.shape[:-1])), int(attr.shape[-1]))      # (-1 is ambiguous when E == 0)
        one = (lambda r: AG.gather_edges(r, ids)) if AG.needs_grad(attr) else (lambda r: AG.gather_edge_values(r.contiguous(), ids))
        rows = [one(flat[i]) for i in range(int(flat.shape[0]))]
        out = rows[0] if attr.dim() == 1 else torch.stack(rows).reshape(tuple(attr.shape[:-1]) + (int(ids.shape[0]),))
    elif attr.dtype == torch.int32 and attr.dim() == 1:
        out = gather_i32(attr.contiguous(), ids)
    else:
        out = torch.index_select(attr, -1, ids.long())      # other dtypes: plumbing, not a hot path
    return torch.cat([out, out], dim=-1) if mirrored else out


def drop_edge(inputs, rate=0.5, force_undirected=False, training=None, seed=None, cache=None, derive_plan=None):
    """
    Reference: tf_geometric/nn/sampling/drop_edge.py:6-52 (same leading arguments).

    :param inputs: List of edge_index and other edge attributes [edge_index, edge_attr, ...]; an attribute is gathered
        along its LAST axis, so [E] and [d, E] both work.  numpy edge_index in -> numpy out.
    :param rate: dropout rate in [0, 1]
    :param force_undirected: keep or drop both directions of an undirected edge together: the result is
        [kept edges with row < col | the same edges flipped]
    :param training: falsy: `inputs` is returned unchanged (the same objects)
    :param seed: None draws a fresh seed per call from torch's generator; an int reproduces the call
    :param cache: the INPUT graph's cache dict: its CSR plan (CACHE_KEY_PLAN) is the parent plan when edge_index carries none.
        Do not hand the same dict to the layers that consume the dropped list — it describes the full graph.
    :param derive_plan: None = DERIVE_PLANS; True / False force the derived / the sorted plan (benchmarks, tests)
    :return: List of dropped edge_index and other dropped edge attributes
    """
    if not training:
        return inputs                                                                              # :18-19
    if rate < 0.0 or rate > 1.0:
        raise ValueError("Dropout probability has to be between 0 and 1, but got {}".format(rate))  # :21-23
    L.require_gpu()
    refuse_capture("drop_edge")
    edge_index, *edge_attrs = inputs
    as_numpy = not isinstance(edge_index, torch.Tensor)
    ei = L.as_i32(edge_index)
    E = int(ei.shape[1]) if ei.dim() == 2 else 0
    for a in edge_attrs:
        if int(np.shape(a)[-1]) != E:
            raise ValueError("an edge attribute has {} entries along its last axis, edge_index has {} edges".format(
                int(np.shape(a)[-1]), E))
    parent = None if as_numpy else _parent_plan(edge_index, E, cache)
    out, edge_id, plan = drop_edge_index(ei, rate, _seed_from_torch() if seed is None else seed, force_undirected,
                                         parent=parent, derive=derive_plan)
    ids = edge_id[:int(edge_id.shape[0]) // 2] if force_undirected else edge_id
    dropped_attrs = [_gather_last_axis(a, ids, bool(force_undirected)) for a in edge_attrs]
    if as_numpy:
        out = out.cpu().numpy()
    elif plan is not None:
        attach_plan(out, plan)      # CsrPlan.from_cache / SparseMatrix.plan pick it up: no sort in the next layer
    return [out] + dropped_attrs
