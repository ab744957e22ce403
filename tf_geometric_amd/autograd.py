# coding=utf-8
"""Differentiable wrappers of the hot-path kernels (the backward pass).

The reference trains with tf.GradientTape over TensorFlow ops (demo/demo_gcn.py:68-77); here the host tensor
library is PyTorch, so the same role is played by torch.autograd.Function objects whose forward AND backward are
C-ABI kernel launches:

  aggregate (sum / mean, weighted)  backward wrt x  = the forward kernel on the transposed (CSR-by-source) plan
                                    backward wrt w  = tfgx_sddmm_f32
  aggregate_project, sage_wide      forward = ONE launch of tfgx_aggregate_gemm_f32 (+ the self half's GEMM); d/dkernel from the
                                    aggregate written beside it (tfgx_gemm_tn_f32), d/d(aggregate) = g @ kernel^T, then as above
    ... over a HalfRows (16-bit)    the SAME three Functions: the table is what the kernel reads (tfgx_segment_reduce_h16 /
                                    tfgx_aggregate_gemm_h16, the float32 route's bits), the tensor autograd differentiates is the
                                    table's float32 gradient sink (_HalfGradSink rounds the summed d/dx to the table's type once)
  aggregate (max)                   training forward saves (max, tie count, arg position); backward = per-edge winner masks +
                                    one gather per edge (tfgx_segment_max_backward_mask_f32, bit-reproducible; ties walked
                                    exactly, TF semantics); MAX_GRADIENT_MODE selects the atomics ("push") or two-gather ("pull") forms
  gat_attention                     tfgx_gat_backward_dst_f32 (dQ) + tfgx_gat_backward_src_f32 (dK, dV)
  linear (x @ W + b, relu)          forward = tfgx_gemm_bias_act_f32; d/dx = the same kernel on W^T (tfgx_transpose_f32);
                                    d/dW, d/db = tfgx_gemm_tn_f32 (MFMA reduction over the node dimension)
  segment_softmax                   forward = tfgx_edge_softmax_f32; backward = out * (g - segsum(out * g)) on the segment kernel
  gcn_norm (tracked edge weights)   forward = the two normalisation kernels on detached data; backward wrt the raw weights =
                                    tfgx_gcn_norm_backward_f32 (row pass, column pass over the transposed plan, edge pass)

The functional API (nn/conv/*.py) routes through these only when torch.is_grad_enabled() and an input requires
grad; inference keeps the fused single-launch paths.
"""
import ctypes
import math

import torch

from . import _lib as L
from .plan import (segment_reduce, can_track, gemm_bias_act, gemm_tn, transpose, SplitRows, gather_friendly_empty,
                   gather_friendly_copy, aggregate_gemm, aggregate_gemm_applies, column_sums, HalfRows)


def needs_grad(*tensors):
    return torch.is_grad_enabled() and any(isinstance(t, (torch.Tensor, HalfRows)) and t.requires_grad for t in tensors)


def _transposed(plan):
    """(transposed plan, t2d) where t2d[j] = forward-CSR position of the edge at transposed-CSR position j."""
    if getattr(plan, "_t2d", None) is None:
        pt = plan.transposed()
        inv = torch.empty_like(plan.perm)
        inv[plan.perm.long()] = torch.arange(plan.num_edges, dtype=torch.int32, device=plan.perm.device)
        plan._t2d = inv[pt.perm.long()].contiguous()
    return plan.transposed(), plan._t2d


def _permute(attr, idx):
    lib = L.require_gpu()
    a = attr.contiguous()
    out = torch.empty_like(a)
    L.check(lib.tfgx_permute_rows_f32(L.ptr(a), L.ptr(idx), int(idx.shape[0]), 1, L.ptr(out), L.stream_ptr()),
            "tfgx_permute_rows_f32")
    return out


def _transposed_weights(plan, w_csr, t2d):
    """w_csr permuted into the transposed plan's order, memoised per (tensor storage, version) on the plan —
    GCN's normalised weights are the same tensor for every layer and every step."""
    if w_csr is None:
        return None
    key = (w_csr.data_ptr(), w_csr._version, int(w_csr.shape[0]))
    cache = plan.__dict__.setdefault("_wt_cache", {})
    hit = cache.get("w")
    if hit is not None and hit[0] == key:
        return hit[1]
    w_t = _permute(w_csr.detach(), t2d)
    cache["w"] = (key, w_t, w_csr)      # keeps w_csr alive so the data_ptr cannot be recycled
    return w_t


import os as _os
# Apply a layer-0 ReLU mask INSIDE the weight-gradient reduction (tfgx_gemm_tn_gated_f32) instead of one masked copy of the
# gradient first.  Same-box A/B at products shape: a wash (GCN step 25.84 / 26.06 vs 25.62 / 26.15 ms, mean SAGE 27.49 /
# 27.67 vs 27.52 / 27.99 ms) — the kernel reads the gate where the copy was written and re-read — so it stays off.
GATED_WEIGHT_GRADIENTS = _os.environ.get("TFGX_GATED_WGRAD", "0") != "0"
# ... and in the fused aggregate -> project layer (round 4, after the weight-gradient kernel's operand loads were rewritten):
GATED_AGGREGATE_PROJECT = _os.environ.get("TFGX_GATED_AGGPROJ", "1") != "0"


def relu_backward(g, out, into=None):
    """g where out > 0, else 0 — ONE pass (tfgx_relu_backward_f32) instead of compare + cast + multiply; g / out / into
    may be column slices of wider matrices."""
    lib = L.require_gpu()
    g2, ldg = L.row_major_2d(g)
    o2, ldo = L.row_major_2d(out)
    M, N = int(g2.shape[0]), int(g2.shape[1])
    res = torch.empty((M, N), dtype=torch.float32, device=g2.device) if into is None else into
    r2, ldr = L.row_major_2d(res)
    assert r2 is res, "relu_backward: `into` must have dense rows"
    L.check(lib.tfgx_relu_backward_f32(L.ptr(g2), ldg, L.ptr(o2), ldo, M, N, L.ptr(res), ldr, L.stream_ptr()),
            "tfgx_relu_backward_f32")
    if into is not None:
        torch.autograd.graph.increment_version(into)
    return res


def _aggregate_grad_x(plan, mean, g, w_csr, self_coef):
    """d/dx of out = (1/cnt) (sum_i w_i x[col_i] + self_coef x): the transposed plan on the same kernel; on a square
    operator the self-loop term self_coef[r] * g[r] rides in that launch's epilogue."""
    if mean:
        scaled = gather_friendly_empty(int(g.shape[0]), int(g.shape[1]), g.device)
        torch.div(g, plan.in_degree().clamp(min=1).to(g.dtype).unsqueeze(1), out=scaled)
        g = scaled
    else:
        g = gather_friendly_copy(g)        # the transposed pass GATHERS rows of g: narrow / odd widths get a padded stride
    pt, t2d = _transposed(plan)
    w_t = _transposed_weights(plan, w_csr, t2d)
    if self_coef is not None and plan.n_dst == plan.n_src:
        return segment_reduce(pt, g, L.SUM, w_csr=w_t, self_coef=self_coef.detach()), g
    gx = segment_reduce(pt, g, L.SUM, w_csr=w_t)
    if self_coef is not None:
        # rectangular plan (n_dst < n_src): only the first n_dst sources carry a self-loop term
        gx[:plan.n_dst] += self_coef.detach().unsqueeze(1) * g
    return gx, g


def _half_source(h, w_csr):
    """(gradient target, edge weights as constants) for a HalfRows source: d/dx goes, in float32, to the table's gradient sink
    (_HalfGradSink; None when the table's source wants no gradient), and the edge weights cannot train."""
    if needs_grad(w_csr):
        raise NotImplementedError("edge weights that require grad are not supported over a 16-bit table (the SDDMM is float32-only)")
    return _half_grad_proxy(h), None if w_csr is None else w_csr.detach()


def _behind_relu(g, out, act, agg=None, upstream=True):
    """(the gradient behind the layer's ReLU, gate): one masked copy of g (tfgx_relu_backward_f32), gate None — or, in layer 0
    of the aggregate -> project operators (nothing upstream wants a gradient, the aggregate was kept for the kernel's), g itself
    and gate = the layer's output: the weight-gradient reductions apply the mask themselves and the masked gradient is never
    written — one 3 x [N, units] pass less (1.45 ms at products shape; the gated kernel costs 0.05 ms more than the plain one
    since its operands moved to raw buffer loads)."""
    gated = act == L.ACT_RELU and agg is not None and not upstream and GATED_AGGREGATE_PROJECT
    if act == L.ACT_RELU and not gated:
        return relu_backward(g, out), None
    return g.contiguous(), (out if gated else None)


def _projection_grads(agg, g, want_b, gate=None):
    """(d/dkernel, d/dbias) of aggregate @ kernel + bias given g: ONE reduction over the node dimension on the saved aggregate
    (agg: kept exactly when the kernel wants its gradient), else the bias' column sums alone."""
    if agg is not None:
        return gemm_tn(agg, g, want_bias=want_b, gate=gate)
    return None, (column_sums(g) if want_b else None)


def _source_grads(plan, mean, x, table, w_csr, self_coef, g, need_x, need_w, need_s, kernel=None):
    """_aggregate_backward for the operators below.  kernel: g is d/d(aggregate @ kernel), so d/d(aggregate) = g @ kernel^T
    first.  The float32 values of the source rows (the SDDMM, the self-loop coefficient's gradient) are x, or a 16-bit table
    widened — only when one of the two is wanted."""
    if kernel is not None:
        g = gemm_bias_act(g, transpose(kernel.detach()))
    if isinstance(table, HalfRows):
        wanted = (need_w and w_csr is not None) or (need_s and self_coef is not None)
        x = table.float() if wanted else None
    return _aggregate_backward(plan, mean, x, w_csr, self_coef, g, need_x, need_w, need_s)


class _Aggregate(torch.autograd.Function):
    """out = act( (1/cnt[r]) * ( sum_{i in row r} w[i] x[col[i]] + self_coef[r] x[r] ) + bias )   (cnt only for mean);
    bias and activation ride in the kernel's epilogue, the ReLU's backward is one masked copy of the gradient."""

    @staticmethod
    def forward(ctx, plan, mean, x, w_csr, self_coef, table=None, bias=None, act=L.ACT_NONE):
        """x: the tensor d/dx goes to.  `table`: what the kernel reads when that is not x itself — x in another source layout
        (a SplitRows: plan.static_rows), or a HalfRows, whose gradient sink x then is (_half_source; tfgx_segment_reduce_h16) —
        same values, same result bits."""
        ctx.plan, ctx.mean, ctx.act, ctx.table = plan, mean, act, table
        out = segment_reduce(plan, x.detach() if table is None else table, L.MEAN if mean else L.SUM,
                             w_csr=None if w_csr is None else w_csr.detach(),
                             self_coef=None if self_coef is None else self_coef.detach(),
                             bias=None if bias is None else bias.detach().contiguous(), act=act)
        ctx.save_for_backward(x, w_csr, self_coef, bias, out if act == L.ACT_RELU else None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w_csr, self_coef, bias, out = ctx.saved_tensors
        _, _, need_x, need_w, need_s, _, need_b, _ = ctx.needs_input_grad
        g, _ = _behind_relu(g, out, ctx.act)
        _, gb = _projection_grads(None, g, bias is not None and need_b)
        gx, gw, gs = _source_grads(ctx.plan, ctx.mean, x, ctx.table, w_csr, self_coef, g, need_x, need_w, need_s)
        return None, None, gx, gw, gs, None, gb, None


def _aggregate_backward(plan, mean, x, w_csr, self_coef, g, need_x, need_w, need_s):
    """(d/dx, d/dw_csr, d/dself_coef) of (1/cnt) (sum_i w_i x[col_i] + self_coef x) given g = d/d(aggregate)."""
    lib = L.require_gpu()
    gx = gw = gs = None
    need_w = need_w and w_csr is not None
    need_s = need_s and self_coef is not None
    if mean and (need_w or need_s) and not need_x:
        g = g / plan.in_degree().clamp(min=1).to(g.dtype).unsqueeze(1)
    if need_x:
        gx, g = _aggregate_grad_x(plan, mean, g, w_csr, self_coef)
    if need_w:
        gw = torch.empty_like(w_csr)
        g2, ldg = L.row_major_2d(g)
        x2, ldx = L.row_major_2d(x.detach())
        hub_w, _ = L.hub_lists(plan)           # hub destinations: their edges are walked chunk-wise
        L.check(lib.tfgx_sddmm_hub_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), plan.n_dst, L.ptr(g2), ldg, L.ptr(x2), ldx,
                                       int(x2.shape[1]), L.ptr(gw), None if hub_w is None else ctypes.byref(hub_w),
                                       L.stream_ptr()), "tfgx_sddmm_hub_f32")
    if need_s:
        gs = (x.detach()[:plan.n_dst] * g).sum(1)
    return gx, gw, gs


class _AggregateProject(torch.autograd.Function):
    """out = act( reduce(plan, x, w, self_coef) @ kernel + bias ) — the aggregate-then-project layers (GCN with units > F,
    the neighbour half of mean / sum GraphSAGE) in ONE forward launch (tfgx_aggregate_gemm_f32; tfgx_aggregate_gemm_h16 over a
    HalfRows: the same bits).  When the kernel needs a gradient the launch also writes the aggregate itself (side output:
    d/dkernel = aggregate^T @ g); the projection still reads it from LDS, so the training forward saves the GEMM's read-back of
    the [N, F] aggregate."""

    @staticmethod
    def forward(ctx, plan, mean, x, w_csr, self_coef, kernel, bias, act, table=None):
        """x, `table`: as in _Aggregate.forward (a SplitRows: same values, same aggregate bits)."""
        need_agg = ctx.needs_input_grad[5]
        agg = torch.empty((plan.n_dst, int(kernel.shape[0])), dtype=torch.float32, device=kernel.device) if need_agg else None
        out = aggregate_gemm(plan, x.detach() if table is None else table, L.MEAN if mean else L.SUM, kernel.detach(),
                             w_csr=None if w_csr is None else w_csr.detach(),
                             self_coef=None if self_coef is None else self_coef.detach(),
                             bias=None if bias is None else bias.detach(), act=act, agg_out=agg, training=True)
        if out is None:
            raise L.TfgxError("_AggregateProject: the fused launch declined (ask plan.aggregate_gemm_applies first)")
        ctx.plan, ctx.mean, ctx.act, ctx.table = plan, mean, act, table
        ctx.save_for_backward(x, w_csr, self_coef, kernel, bias, agg, out if act == L.ACT_RELU else None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w_csr, self_coef, kernel, bias, agg, out = ctx.saved_tensors
        _, _, need_x, need_w, need_s, _, need_b, _, _ = ctx.needs_input_grad
        upstream = need_x or need_w or need_s
        g, gate = _behind_relu(g, out, ctx.act, agg, upstream)
        gk, gb = _projection_grads(agg, g, bias is not None and need_b, gate)
        gx = gw = gs = None
        if upstream:
            gx, gw, gs = _source_grads(ctx.plan, ctx.mean, x, ctx.table, w_csr, self_coef, g, need_x, need_w, need_s, kernel)
        return None, None, gx, gw, gs, gk, gb, None, None


def aggregate_project(plan, x, op, kernel, w_csr=None, self_coef=None, bias=None, act=L.ACT_NONE, rows=None):
    """Differentiable act(reduce(plan, x) @ kernel + bias) on the fused launch, or None when it does not take the shape
    (the caller then composes aggregate + linear).  rows: x's static layout (plan.static_rows) or None / x itself.
    x may be a HalfRows (tfgx_aggregate_gemm_h16; rows is not consulted; trainable edge weights: NotImplementedError)."""
    table = x if isinstance(x, HalfRows) else (rows if isinstance(rows, SplitRows) else None)
    if op not in (L.SUM, L.MEAN) or not aggregate_gemm_applies(x if table is None else table, kernel, op):
        return None
    if table is x:
        x, w_csr = _half_source(x, w_csr)
    return _AggregateProject.apply(plan, op == L.MEAN, x, w_csr, self_coef, L.as_f32(kernel),
                                   None if bias is None else L.as_f32(bias), act, table)


class _SageWide(torch.autograd.Function):
    """h = act([xs @ ks | reduce(w * x[col]) @ kn] + bias): mean / sum GraphSAGE, concat form, aggregation first (ku >= F:
    nn/conv/graph_sage.py:34-58 with demo_graph_sage.py:29-30's units=256).  The neighbour half is ONE launch
    (tfgx_aggregate_gemm_f32 / _h16 straight into its half of h, aggregate written beside it for d/dkn), the self half the GEMM."""

    @staticmethod
    def forward(ctx, plan, mean, x, xs, ks, kn, w_csr, bias, act, table=None, self_table=None):
        """x, `table`: as in _Aggregate.forward.  xs: what the self half reads — x itself, or over a HalfRows the widened
        table (widen), whose gradient reaches the same sink: the two halves' d/dx are summed by autograd either way.
        `self_table`: a HalfRows declared a GEMM operand, which the self half reads in place of a widened copy (xs is then its
        gradient sink, like x)."""
        xr = _rows_of(xs, self_table)
        n, F, na, nb = int(xr.shape[0]), int(kn.shape[0]), int(ks.shape[1]), int(kn.shape[1])
        h = torch.empty((n, na + nb), dtype=torch.float32, device=kn.device)
        bd = None if bias is None else bias.detach().contiguous()
        agg = torch.empty((n, F), dtype=torch.float32, device=kn.device) if ctx.needs_input_grad[5] else None
        got = aggregate_gemm(plan, x.detach() if table is None else table, L.MEAN if mean else L.SUM, kn.detach(),
                             w_csr=None if w_csr is None else w_csr.detach(),
                             bias=None if bd is None else bd[na:].contiguous(), act=act, out=h[:, na:], agg_out=agg, training=True)
        if got is None:
            raise L.TfgxError("_SageWide: the fused launch declined (ask plan.aggregate_gemm_applies first)")
        gemm_bias_act(xr, ks.detach(), bias=None if bd is None else bd[:na], act=act, out=h[:, :na])
        ctx.plan, ctx.mean, ctx.act, ctx.na, ctx.table, ctx.self_table = plan, mean, act, na, table, self_table
        ctx.save_for_backward(xs, ks, kn, w_csr, bias, agg, h if act == L.ACT_RELU else None)
        return h

    @staticmethod
    def backward(ctx, g):
        xs, ks, kn, w_csr, bias, agg, h = ctx.saved_tensors
        _, _, need_x, need_xs, need_ks, _, _, need_b, _, _, _ = ctx.needs_input_grad
        na, upstream, want_b = ctx.na, need_x or need_xs, bias is not None and need_b
        g, gate = _behind_relu(g, h, ctx.act, agg, upstream)          # gated: layer 0, x carries no gradient
        gs, gn = g[:, :na], g[:, na:]
        gxs, gks, gba = _linear_grads(ctx.self_table if ctx.self_table is not None else xs, ks, gs, upstream, need_ks, want_b,
                                      gate=None if gate is None else gate[:, :na])
        gkn, gbb = _projection_grads(agg, gn, want_b, None if gate is None else gate[:, na:])
        gx = None
        if upstream:
            gx, _, _ = _source_grads(ctx.plan, ctx.mean, None, ctx.table, w_csr, None, gn, True, False, False, kn)
        gb = torch.cat([gba, gbb]) if want_b else None
        return None, None, gx if need_x else None, gxs if need_xs else None, gks, gkn, None, gb, None, None, None


def sage_wide(plan, op, x, ks, kn, w_csr=None, bias=None, act=L.ACT_NONE, rows=None):
    """Differentiable mean / sum GraphSAGE layer body (concat form, aggregation first) with the neighbour half on the fused
    launch, or None when it does not take the shape.  Edge weights are constants here (trainable ones take the un-fused route).
    rows: x's static layout (plan.static_rows) or None / x itself.
    x may be a HalfRows (rows is not consulted; the self half reads the widened table, or the table itself when it was declared
    a GEMM operand; trainable edge weights: NotImplementedError)."""
    table = x if isinstance(x, HalfRows) else (rows if isinstance(rows, SplitRows) else None)
    if op not in (L.SUM, L.MEAN) or not aggregate_gemm_applies(x if table is None else table, kn, op):
        return None
    xs, self_table = x, None
    if table is x:
        x, w_csr = _half_source(table, w_csr)
        if table.gemm_operand:      # the self half reads the table itself; its d/dx reaches the same sink as the aggregation's
            xs, self_table = x, table
        else:
            xs = widen(table)
    return _SageWide.apply(plan, op == L.MEAN, x, xs, L.as_f32(ks), L.as_f32(kn), w_csr,
                           None if bias is None else L.as_f32(bias), act, table, self_table)


# Gradient of max aggregation (tf.math.unsorted_segment_max, ties share evenly):
#   "mask"  (default) per-edge winner bit masks from the saved arg positions, one gather per edge, bit-reproducible
#   "push"  N*F float atomics from the saved arg positions (summation order = arrival order)
#   "pull"  two row gathers per edge over the transposed plan, bit-reproducible, needs nothing saved (hub graphs)
MAX_GRADIENT_MODE = "mask"
DETERMINISTIC_MAX_GRADIENT = False     # legacy switch: True forces "pull"


def _max_mode():
    return "pull" if DETERMINISTIC_MAX_GRADIENT else MAX_GRADIENT_MODE


class _AggregateMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, x, w_csr, passes=None):
        """`passes` (the sharded path, dist/sharded.py::tracked_max_passes): callable(x2, w, out, packed) that runs the
        tracked forward as several launches over consecutive sub-spans of every row (merged in the kernel epilogue) —
        same (out, packed) as the single launch below, so the backward does not know the difference."""
        lib = L.require_gpu()
        x2, ldx = L.row_major_2d(x.detach())
        F = int(x2.shape[1])
        argpos = None
        wd = None if w_csr is None else w_csr.detach()
        packed = None
        if passes is not None:
            out = torch.empty((plan.n_dst, F), dtype=torch.float32, device=x2.device)
            packed = torch.empty((plan.n_dst, F), dtype=torch.int32, device=x2.device)
            passes(x2, wd, out, packed)
            count = None
            ctx.halo_first = getattr(passes, "halo_first", None)     # (n_own, [(lo, hi) per round], callable(j, gx)): see backward
        elif _max_mode() == "mask" and can_track(plan, x2, ldx):
            # the tuned forward walk (8 gathered rows in flight per lane group) with the tie count and the position of the
            # first maximal edge tracked online and written PACKED (one uint32 per element instead of a float count array
            # and an int32 position array): what the mask-form backward reads
            out = torch.empty((plan.n_dst, F), dtype=torch.float32, device=x2.device)
            packed = torch.empty((plan.n_dst, F), dtype=torch.int32, device=x2.device)
            segment_reduce(plan, x2, L.MAX, w_csr=wd, out=out, track=packed)
            count = None
        elif plan.hub_info() is None:
            # one pass: row maxima AND how many edges attain each (the tie count TF's gradient divides by)
            out = torch.empty((plan.n_dst, F), dtype=torch.float32, device=x2.device)
            count = torch.empty_like(out)
            push_ok = _max_mode() in ("mask", "push") and F % 4 == 0 and ldx % 4 == 0 and x2.data_ptr() % 16 == 0
            if push_ok:       # ... and WHICH edge attains it first: the backward becomes N*F atomics instead of E*F gathers
                argpos = torch.empty((plan.n_dst, F), dtype=torch.int32, device=x2.device)
                L.check(lib.tfgx_segment_max_with_arg_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), L.ptr(wd), plan.n_dst,
                                                          L.ptr(x2), ldx, F, L.ptr(out), F, L.ptr(count), F,
                                                          L.ptr(argpos), F, L.stream_ptr()),
                        "tfgx_segment_max_with_arg_f32")
            else:
                L.check(lib.tfgx_segment_max_with_count_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), L.ptr(wd), plan.n_dst,
                                                            L.ptr(x2), ldx, F, L.ptr(out), F, L.ptr(count), F,
                                                            L.stream_ptr()), "tfgx_segment_max_with_count_f32")
        else:   # skewed graph: the chunked forward keeps long rows off one lane group; count in the backward
            out = segment_reduce(plan, x2, L.MAX, w_csr=wd)
            count = None
        ctx.plan, ctx.count, ctx.argpos, ctx.mode, ctx.packed = plan, count, argpos, _max_mode(), packed
        if passes is None:
            ctx.halo_first = None
        ctx.save_for_backward(x, w_csr, out)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = L.require_gpu()
        plan = ctx.plan
        x, w_csr, out = ctx.saved_tensors
        x2, ldx = L.row_major_2d(x.detach())
        g2, ldg = L.row_major_2d(g.contiguous())
        F = int(x2.shape[1])
        count = ctx.count
        packed = ctx.packed

        def unpack_count():
            return ((packed.to(torch.int64) & 0xFFFFFFFF) >> 16).to(torch.float32)
        if count is None and packed is None:          # skewed graph: hub rows counted chunk-wise
            count = torch.empty_like(out)
            hub_c, nc_c = L.hub_lists(plan)
            sc_c = torch.empty(max(nc_c * F, 1), dtype=torch.float32, device=x2.device) if hub_c is not None else None
            L.check(lib.tfgx_segment_max_count_hub_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), L.ptr(w_csr), plan.n_dst,
                                                       L.ptr(x2), ldx, F, L.ptr(out), F, L.ptr(count), F,
                                                       None if hub_c is None else ctypes.byref(hub_c), L.ptr(sc_c),
                                                       L.stream_ptr()), "tfgx_segment_max_count_hub_f32")
        gx = None
        if ctx.needs_input_grad[1]:
            gx = torch.empty((int(x2.shape[0]), F), dtype=torch.float32, device=x2.device)   # dense: ld = F below
            aligned = (ctx.argpos is not None or packed is not None) and ldg % 4 == 0 and g2.data_ptr() % 16 == 0
            pt_hub, nc_t = L.hub_lists(_transposed(plan)[0])
            if pt_hub is not None:
                aligned = False        # hub SOURCES: the per-source walks of the mask / push forms would serialise; pull, chunked
            if packed is not None and not aligned:
                count = unpack_count()             # rare fall-back to the pull form: it wants the float count array
            if aligned and packed is not None:
                pt, t2d = _transposed(plan)
                w_t = _transposed_weights(plan, w_csr, t2d)
                ws_bytes = lib.tfgx_segment_max_backward_mask_workspace_bytes(plan.n_dst, plan.num_edges, F)
                ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x2.device)
                n_table = int(x2.shape[0])

                def run(phases, lo, hi):       # masks built / applied to source rows [lo, hi) of the table
                    L.check(lib.tfgx_segment_max_backward_mask_phases_f32(
                        L.ptr(plan.row_ptr), L.ptr(plan.col), L.ptr(None if w_csr is None else w_csr.detach()), plan.n_dst,
                        plan.num_edges, L.ptr(x2), ldx, F, L.ptr(out), F, L.ptr(g2), ldg, None, F, L.ptr(packed), F,
                        pt.row_ptr.data_ptr() + 4 * lo, L.ptr(pt.col), L.ptr(w_t), L.ptr(t2d), hi - lo,
                        gx.data_ptr() + 4 * F * lo, F, L.ptr(ws), ws_bytes, phases, L.stream_ptr()),
                        "tfgx_segment_max_backward_mask_phases_f32 (packed)")
                hf = getattr(ctx, "halo_first", None)
                if hf is not None and 0 < hf[0] < n_table:
                    # sharded table [own | halo]: the halo rows' gradients belong to peers — compute them first, window by
                    # window (one per exchange round), and let each window travel (reverse exchange on the communication
                    # stream) while the following windows and the own rows' part run
                    run(1, 0, 0)                                   # masks + g / count, once
                    for j, (lo, hi) in enumerate(hf[1]):
                        if hi > lo:
                            run(2, lo, hi)
                        hf[2](j, gx)
                    run(2, 0, hf[0])
                else:
                    run(3, 0, n_table)
            elif aligned and ctx.mode == "mask":
                pt, t2d = _transposed(plan)
                w_t = _transposed_weights(plan, w_csr, t2d)
                ws_bytes = lib.tfgx_segment_max_backward_mask_workspace_bytes(plan.n_dst, plan.num_edges, F)
                ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x2.device)
                L.check(lib.tfgx_segment_max_backward_mask_f32(
                    L.ptr(plan.row_ptr), L.ptr(plan.col), L.ptr(None if w_csr is None else w_csr.detach()), plan.n_dst,
                    plan.num_edges, L.ptr(x2), ldx, F, L.ptr(out), F, L.ptr(g2), ldg, L.ptr(count), F, L.ptr(ctx.argpos), F,
                    L.ptr(pt.row_ptr), L.ptr(pt.col), L.ptr(w_t), L.ptr(t2d), int(x2.shape[0]), L.ptr(gx), F, L.ptr(ws),
                    ws_bytes, L.stream_ptr()), "tfgx_segment_max_backward_mask_f32")
            elif aligned:
                L.check(lib.tfgx_segment_max_backward_push_f32(
                    L.ptr(plan.row_ptr), L.ptr(plan.col), L.ptr(None if w_csr is None else w_csr.detach()), plan.n_dst,
                    int(x2.shape[0]), L.ptr(x2), ldx, F, L.ptr(out), F, L.ptr(g2), ldg, L.ptr(count), F,
                    L.ptr(ctx.argpos), F, L.ptr(gx), F, L.stream_ptr()), "tfgx_segment_max_backward_push_f32")
            else:
                pt, t2d = _transposed(plan)
                w_t = _transposed_weights(plan, w_csr, t2d)
                gn = torch.empty_like(out)          # workspace: g / count per destination row
                sc_t = torch.empty(max(nc_t * F, 1), dtype=torch.float32, device=x2.device) if pt_hub is not None else None
                L.check(lib.tfgx_segment_max_backward_hub_f32(
                    L.ptr(pt.row_ptr), L.ptr(pt.col), L.ptr(w_t), pt.n_dst, L.ptr(x2), ldx, F, L.ptr(out), F, L.ptr(g2), ldg,
                    L.ptr(count), F, L.ptr(gx), F, plan.n_dst, L.ptr(gn), None if pt_hub is None else ctypes.byref(pt_hub),
                    L.ptr(sc_t), L.stream_ptr()), "tfgx_segment_max_backward_hub_f32")
        gw = None
        if w_csr is not None and ctx.needs_input_grad[2]:
            if count is None:
                count = unpack_count()
            gn2 = g2 / count.clamp(min=1.0)          # TF splits the gradient evenly among tied maxima
            gw = torch.empty_like(w_csr)
            L.check(lib.tfgx_segment_max_backward_w_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), L.ptr(w_csr.detach()),
                                                        plan.n_dst, L.ptr(x2), ldx, F, L.ptr(out), F, L.ptr(gn2), F,
                                                        L.ptr(gw), L.stream_ptr()), "tfgx_segment_max_backward_w_f32")
        return None, gx, gw, None


POOL_MLP_MAX_FUSED = _os.environ.get("TFGX_POOL_MLP_MAX_FUSED", "1") != "0"     # developer A/B


def pool_mlp_max_applies(plan, x, kernel):
    """Can the pooling MLP + max of max-pool GraphSAGE run as autograd._PoolMlpMax with the destination-major weight
    gradient (tfgx_pool_mlp_max_wgrad_f32)?  Dense float32 features that carry NO gradient (layer 0 of a model), shapes the
    kernel is instantiated for, and a plan whose rows the tracked forward can take."""
    if not POOL_MLP_MAX_FUSED or not isinstance(x, torch.Tensor) or x.requires_grad or not torch.is_grad_enabled():
        return False
    lib = L.require_gpu()
    F_in, Fp = int(x.shape[1]), int(kernel.shape[1])
    if not lib.tfgx_pool_mlp_max_wgrad_applies(F_in, Fp):
        return False
    x2, ldx = L.row_major_2d(x)
    if ldx % 4 != 0 or x2.data_ptr() % 16 != 0 or plan.n_dst != plan.n_src:
        return False
    from .plan import gather_friendly_ld
    return _max_mode() == "mask" and can_track(plan, _FutureRows(Fp), gather_friendly_ld(Fp))


class _FutureRows(object):
    """What plan.can_track looks at, for the [n, F] hidden rows that do not exist yet: their width and (torch's allocations are
    256-byte aligned) an aligned address."""

    def __init__(self, F):
        self.shape = (0, F)

    def data_ptr(self):
        return 0


class _PoolMlpMax(torch.autograd.Function):
    """red = max over in-edges of relu(x W + b)[col] — the pooling MLP and the max of max-pool GraphSAGE
    (nn/conv/graph_sage.py:260-269) as ONE operator for features that carry no gradient.  Forward: the MFMA GEMM (bias + ReLU
    in its epilogue, rows at the gather-friendly stride) and the tracked max.  Backward: dW, db straight from the destination
    rows (tfgx_pool_mlp_max_wgrad_f32) — the gradient of the hidden rows, the per-edge winner masks, the ReLU-mask pass and the
    reduction x^T dh of the composed form are never computed."""

    @staticmethod
    def forward(ctx, plan, x, kernel, bias):
        n, Fp = int(x.shape[0]), int(kernel.shape[1])
        h = gemm_bias_act(x.detach(), kernel.detach(), bias=None if bias is None else bias.detach(), act=L.ACT_RELU,
                          out=gather_friendly_empty(n, Fp, x.device))
        red = torch.empty((plan.n_dst, Fp), dtype=torch.float32, device=x.device)
        packed = torch.empty((plan.n_dst, Fp), dtype=torch.int32, device=x.device)
        segment_reduce(plan, h, L.MAX, out=red, track=packed)
        ctx.plan = plan
        ctx.save_for_backward(x, h, red, packed, bias)
        return red

    @staticmethod
    def backward(ctx, g):
        lib = L.require_gpu()
        plan = ctx.plan
        x, h, red, packed, bias = ctx.saved_tensors
        x2, ldx = L.row_major_2d(x.detach())
        h2, ldh = L.row_major_2d(h)
        g2, ldg = L.row_major_2d(g.contiguous())
        F_in, Fp = int(x2.shape[1]), int(h2.shape[1])
        dW = torch.empty((F_in, Fp), dtype=torch.float32, device=x2.device)
        db = torch.empty(Fp, dtype=torch.float32, device=x2.device) if bias is not None else None
        # the launch's work items depend on the graph and on (F_in, Fp) alone: built once, kept on the plan
        items = plan.__dict__.setdefault("_pool_wgrad_items", {})
        key = (F_in, Fp)
        if key not in items:
            nb = lib.tfgx_pool_mlp_max_wgrad_plan_bytes(plan.n_dst, plan.num_edges, F_in, Fp)
            buf = torch.empty(max(nb, 1), dtype=torch.uint8, device=x2.device)
            L.check(lib.tfgx_pool_mlp_max_wgrad_plan(L.ptr(plan.row_ptr), plan.n_dst, plan.num_edges, F_in, Fp, L.ptr(buf), nb,
                                                     L.stream_ptr()), "tfgx_pool_mlp_max_wgrad_plan")
            items[key] = buf
        ws_bytes = lib.tfgx_pool_mlp_max_wgrad_workspace_bytes(plan.n_dst, F_in, Fp)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x2.device)
        L.check(lib.tfgx_pool_mlp_max_wgrad_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), plan.n_dst, plan.num_edges, L.ptr(x2), ldx, F_in,
                                                L.ptr(h2), ldh, L.ptr(red), Fp, L.ptr(packed), Fp, L.ptr(g2), ldg, Fp,
                                                L.ptr(items[key]), L.ptr(dW), Fp, L.ptr(db), L.ptr(ws), ws_bytes, L.stream_ptr()),
                "tfgx_pool_mlp_max_wgrad_f32")
        need = ctx.needs_input_grad
        return None, None, (dW if need[2] else None), (db if (bias is not None and need[3]) else None)


def pool_mlp_max(plan, x, kernel, bias):
    """max over in-edges of relu(x @ kernel + bias)[col]; differentiable w.r.t. kernel and bias only (ask pool_mlp_max_applies)."""
    return _PoolMlpMax.apply(plan, L.as_f32(x), L.as_f32(kernel), None if bias is None else L.as_f32(bias))


class _HalfGradSink(torch.autograd.Function):
    """The ONE place the gradient of a HalfRows.from_tensor(t) reaches t: every use of the table (aggregation, widening) sends
    its float32 gradient to the same float32 [n, F] proxy (a stride-0 view: no table is allocated), autograd sums them in
    float32, and this node rounds the sum to t.dtype once, to nearest even, as the last step."""

    @staticmethod
    def forward(ctx, src):
        ctx.dtype, ctx.device = src.dtype, src.device
        return torch.zeros((1, 1), dtype=torch.float32, device=L.device()).expand(int(src.shape[0]), int(src.shape[1]))

    @staticmethod
    def backward(ctx, g):
        lib = L.require_gpu()
        g, ldg = L.row_major_2d(L.as_f32(g))
        n, F = int(g.shape[0]), int(g.shape[1])
        gx = torch.empty((n, F), dtype=ctx.dtype, device=g.device)       # dense: no copy off a padded stride afterwards
        L.check(lib.tfgx_rows_f32_to_h16(L.ptr(g), ldg, n, F, L.ptr(gx), max(F, 1), L.H16_DTYPES[ctx.dtype], L.stream_ptr()),
                "tfgx_rows_f32_to_h16")
        return gx if gx.device == ctx.device else gx.to(ctx.device)


def _half_grad_proxy(h):
    """The float32 gradient sink of a HalfRows whose source requires grad (one per HalfRows), else None."""
    if not needs_grad(h):
        return None
    proxy = getattr(h, "_grad_proxy", None)
    if proxy is None:
        proxy = h._grad_proxy = _HalfGradSink.apply(h.source)
    return proxy


class _WidenHalf(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, proxy):
        return h.float()

    @staticmethod
    def backward(ctx, g):
        return None, g


def widen(h):
    """h.float() with a gradient: d/dt of HalfRows.from_tensor(t) flows through the widened tensor too (the self / identity
    terms of aggregate_neighbors and the GraphSAGE layers), summed in float32 with the aggregation's and rounded once."""
    proxy = _half_grad_proxy(h)
    return h.float() if proxy is None else _WidenHalf.apply(h, proxy)


def _aggregate_half(plan, h, op, w_csr, self_coef, bias, act, rows, max_passes):
    """What aggregate checks for a HalfRows; max aggregation (inference only) is answered here, sum / mean with None."""
    if rows is not None or max_passes is not None:
        raise TypeError("aggregate on a HalfRows takes neither rows= (the split-row layouts) nor max_passes= (the tracked max)")
    if op != L.MAX:
        return None
    if needs_grad(h, w_csr, self_coef, bias):
        raise NotImplementedError("max aggregation over a 16-bit table is inference-only (the kernel keeps no track table)")
    return segment_reduce(plan, h, L.MAX, w_csr=w_csr, self_coef=self_coef, bias=bias, act=act)


def aggregate(plan, x, op, w_csr=None, self_coef=None, rows=None, bias=None, act=L.ACT_NONE, max_passes=None):
    """Differentiable gather-scale-segment-reduce (sum / mean / max) on `plan`; sum / mean take the layer's bias and
    ReLU in the kernel epilogue (bias: a tensor that may require grad).  x may be a HalfRows (sum / mean; max without grad)."""
    table = rows if isinstance(rows, SplitRows) else None
    if isinstance(x, HalfRows):
        out = _aggregate_half(plan, x, op, w_csr, self_coef, bias, act, rows, max_passes)
        if out is not None:
            return out
        table = x
        x, w_csr = _half_source(table, w_csr)
    elif op == L.MAX:
        if self_coef is not None:
            raise NotImplementedError("max aggregation with an implicit self-loop is inference-only")
        h = _AggregateMax.apply(plan, x, w_csr, max_passes)
        if bias is not None:
            h = bias_add(h, bias)
        return torch.relu(h) if act == L.ACT_RELU else h
    return _Aggregate.apply(plan, op == L.MEAN, x, w_csr, self_coef, table, bias, act)


def _gemm_source(x):
    """(the tensor in x's autograd position, the table the GEMMs read) of a dense operand.  A float32 tensor: (x, None).  A
    HalfRows: its float32 gradient sink (_half_grad_proxy; None when the table's source wants no gradient — d/dx is then not
    computed) and the table itself, which the operators keep on ctx as an attribute: it is no tensor to save_for_backward."""
    if isinstance(x, HalfRows):
        return _half_grad_proxy(x), x
    return x, None


def _rows_of(x, table):
    """What the kernels read: the table when there is one, else the detached tensor."""
    return table if table is not None else x.detach()


def _linear_grads(x, kernel, g, need_x, need_k, need_b, gate=None):
    """(d/dx, d/dkernel, d/dbias) of x @ kernel + bias given g (which may be a column slice of a wider gradient).
    `gate`: the layer's ReLU output when g is still UN-masked — only valid without d/dx (the reduction kernel applies
    the mask in registers; layer 0 of every model, whose input carries no gradient)."""
    assert gate is None or not need_x
    # d/dx = g @ kernel^T: the forward MFMA kernel with the (small) transposed kernel as B
    gx = gemm_bias_act(g, transpose(kernel.detach())) if need_x else None
    # d/dkernel = x^T @ g and d/dbias = column sums of g: ONE reduction over the node dimension (tfgx_gemm_tn_f32)
    gk = gb = None
    if need_k or need_b:
        gk, gb = gemm_tn(x if isinstance(x, HalfRows) else x.detach(), g, want_bias=need_b, gate=gate)
        if not need_k:
            gk = None
    return gx, gk, gb


class _DualLinear(torch.autograd.Function):
    """h = act([x @ ka | r @ kb] + bias): GraphSAGE's concat of the self and neighbour projections (graph_sage.py:43-58)
    with both GEMMs writing straight into their halves of the output (bias + activation in the epilogues) — no concat,
    no bias add, no activation pass; the backward slices the (masked) gradient by column views."""

    @staticmethod
    def forward(ctx, x, ka, r, kb, bias, act, table=None):
        """x, `table`: _gemm_source of the self operand (a HalfRows: the GEMM and the weight gradient read the table)."""
        xr = _rows_of(x, table)
        n, na, nb = int(xr.shape[0]), int(ka.shape[1]), int(kb.shape[1])
        h = torch.empty((n, na + nb), dtype=torch.float32, device=ka.device)
        bd = None if bias is None else bias.detach().contiguous()
        gemm_bias_act(xr, ka.detach(), bias=None if bd is None else bd[:na], act=act, out=h[:, :na])
        gemm_bias_act(r.detach(), kb.detach(), bias=None if bd is None else bd[na:], act=act, out=h[:, na:])
        ctx.act, ctx.na, ctx.table = act, na, table
        ctx.save_for_backward(x, ka, r, kb, bias, h if act == L.ACT_RELU else None)
        return h

    @staticmethod
    def backward(ctx, g):
        x, ka, r, kb, bias, h = ctx.saved_tensors
        na = ctx.na
        need = ctx.needs_input_grad
        relu = ctx.act == L.ACT_RELU
        # no d/dx, d/dr wanted (layer 0: the inputs are data): the ReLU mask is applied inside the reduction kernels
        gated = relu and not need[0] and not need[2] and GATED_WEIGHT_GRADIENTS
        g = relu_backward(g, h) if (relu and not gated) else g.contiguous()
        want_b = bias is not None and need[4]
        gx, gka, gba = _linear_grads(ctx.table if ctx.table is not None else x, ka, g[:, :na], need[0], need[1], want_b,
                                     gate=h[:, :na] if gated else None)
        gr, gkb, gbb = _linear_grads(r, kb, g[:, na:], need[2], need[3], want_b, gate=h[:, na:] if gated else None)
        gb = torch.cat([gba, gbb]) if want_b else None
        return gx, gka, gr, gkb, gb, None, None


class _SageNarrow(torch.autograd.Function):
    """h = act([x @ ks | reduce(w * (x @ kn)[col])] + bias): mean / sum GraphSAGE with the neighbour projection run
    BEFORE the (linear) reduction (nn/conv/graph_sage._self_neighbor_sage), both halves written in place — the GEMM's and
    the aggregation's epilogues carry bias + activation, nothing is concatenated."""

    @staticmethod
    def forward(ctx, plan, mean, x, ks, kn, w_csr, bias, act, table=None):
        """x, `table`: _gemm_source of the features (a HalfRows: both projections and the weight gradient read the table)."""
        xr = _rows_of(x, table)
        n, na, nb = int(xr.shape[0]), int(ks.shape[1]), int(kn.shape[1])
        h = torch.empty((n, na + nb), dtype=torch.float32, device=ks.device)
        bd = None if bias is None else bias.detach().contiguous()
        gemm_bias_act(xr, ks.detach(), bias=None if bd is None else bd[:na], act=act, out=h[:, :na])
        z = gemm_bias_act(xr, kn.detach(), out=gather_friendly_empty(n, nb, ks.device))
        segment_reduce(plan, z, L.MEAN if mean else L.SUM, w_csr=None if w_csr is None else w_csr.detach(),
                       out=h[:, na:], act=act, bias=None if bd is None else bd[na:].contiguous())
        ctx.plan, ctx.mean, ctx.act, ctx.na, ctx.table = plan, mean, act, na, table
        ctx.save_for_backward(x, ks, kn, w_csr, bias, h if act == L.ACT_RELU else None)
        return h

    @staticmethod
    def backward(ctx, g):
        """D = [masked g of the self half | d/dz of the neighbour half] is assembled in ONE buffer, so that both kernels'
        gradients come from one reduction over x (x^T @ D = [d/dks | d/dkn]) and d/dx from one GEMM (D @ [ks | kn]^T)
        instead of two of each plus an add."""
        x, ks, kn, w_csr, bias, h = ctx.saved_tensors
        plan, na, need = ctx.plan, ctx.na, ctx.needs_input_grad
        n, nb = int(g.shape[0]), int(kn.shape[1])
        relu = ctx.act == L.ACT_RELU
        want_b = bias is not None and need[6]
        D = torch.empty((n, na + nb), dtype=torch.float32, device=g.device)
        gn = gather_friendly_empty(n, nb, g.device)      # gathered by the transposed pass: line-friendly stride
        if relu:
            relu_backward(g[:, :na], h[:, :na], into=D[:, :na])
            relu_backward(g[:, na:], h[:, na:], into=gn)
        else:
            D[:, :na] = g[:, :na]
            gn.copy_(g[:, na:])
        gbb = column_sums(gn) if want_b else None
        if ctx.mean:
            gn.div_(plan.in_degree().clamp(min=1).to(gn.dtype).unsqueeze(1))
        pt, t2d = _transposed(plan)
        segment_reduce(pt, gn, L.SUM, w_csr=_transposed_weights(plan, w_csr, t2d), out=D[:, na:])
        gks = gkn = gb = gx = None
        if need[3] or need[4] or want_b:
            gW, gb_all = gemm_tn(_rows_of(x, ctx.table), D, want_bias=want_b)
            gks, gkn = (gW[:, :na] if need[3] else None), (gW[:, na:] if need[4] else None)
            if want_b:
                gb = torch.cat([gb_all[:na], gbb])
        if need[2]:
            gx = gemm_bias_act(D, transpose(torch.cat([ks.detach(), kn.detach()], dim=1)))
        return None, None, gx, gks, gkn, None, gb, None, None


def sage_narrow(plan, op, x, ks, kn, w_csr=None, bias=None, act=L.ACT_NONE):
    """Fused differentiable mean / sum GraphSAGE layer body (concat form, neighbour projection first).  The edge weights
    are treated as constants (callers route trainable edge weights through the un-fused operators)."""
    x, table = _gemm_source(x)
    return _SageNarrow.apply(plan, op == L.MEAN, x, L.as_f32(ks), L.as_f32(kn), w_csr,
                             None if bias is None else L.as_f32(bias), act, table)


def dual_linear(x, ka, r, kb, bias=None, act=L.ACT_NONE):
    """x (the self operand) may be a HalfRows."""
    x, table = _gemm_source(x)
    return _DualLinear.apply(x, L.as_f32(ka), r, L.as_f32(kb), None if bias is None else L.as_f32(bias), act, table)


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, bias, act, gathered=False, table=None):
        """gathered=True: the rows are gathered by an aggregation next — written at a line-friendly stride.
        x, `table`: _gemm_source of the operand (a HalfRows: the GEMM and the weight gradient read the table)."""
        xr = _rows_of(x, table)
        dst = gather_friendly_empty(int(xr.shape[0]), int(kernel.shape[1]), kernel.device) if gathered else None
        out = gemm_bias_act(xr, kernel.detach(), bias=None if bias is None else bias.detach(), act=act, out=dst)
        ctx.act, ctx.table = act, table
        ctx.save_for_backward(x, kernel, bias, out)
        return out

    @staticmethod
    def backward(ctx, g):
        x, kernel, bias, out = ctx.saved_tensors
        relu = ctx.act == L.ACT_RELU
        gated = relu and not ctx.needs_input_grad[0] and GATED_WEIGHT_GRADIENTS      # no d/dx: mask applied inside the reduction kernel
        g = relu_backward(g, out) if (relu and not gated) else g.contiguous()
        gx, gk, gb = _linear_grads(ctx.table if ctx.table is not None else x, kernel, g, ctx.needs_input_grad[0],
                                   ctx.needs_input_grad[1], bias is not None and ctx.needs_input_grad[2], gate=out if gated else None)
        return gx, gk, gb, None, None, None


def linear(x, kernel, bias=None, act=L.ACT_NONE, gathered=False):
    """act(x @ kernel + bias): forward on the MFMA kernel, differentiable.  gathered=True when an aggregation reads the
    result next (plan.gather_friendly_ld).  x may be a HalfRows: the forward and the weight gradient read the table
    (tfgx_gemm_bias_act_cols_ws_h16 / tfgx_gemm_tn_gated_h16); d/dx is computed only when the table's source requires grad."""
    x, table = _gemm_source(x)
    return _Linear.apply(x, L.as_f32(kernel), None if bias is None else L.as_f32(bias), act, gathered, table)


class _ProjectQKV(torch.autograd.Function):
    """Q = act(x Wq + bq), K = act(x Wk + bk), V = x W (nn/conv/gat.py:52-70) as ONE differentiable operator: the forward reads
    x twice ([Q | K] in one GEMM when they share the activation, V in a second one with its gather-friendly stride), the
    backward ONCE — the masked dQ, dK and dV are laid side by side in one [n, 2A + U] matrix D, so that all three weight
    gradients and both bias gradients come from one reduction over x (x^T D) and d/dx from one GEMM (D [Wq | Wk | W]^T).
    Three separate linear layers read the 561 MB Reddit-shaped x six times per training step; this reads it three times."""

    @staticmethod
    def forward(ctx, x, wq, bq, wk, bk, wv, act, table=None):
        """x, `table`: _gemm_source of the features (a HalfRows: the projections and the weight gradient read the table)."""
        xd = _rows_of(x, table)
        n, A, U = int(xd.shape[0]), int(wq.shape[1]), int(wv.shape[1])
        w_qk = torch.cat([wq.detach(), wk.detach()], dim=1).contiguous()
        b_qk = None if bq is None else torch.cat([bq.detach().reshape(-1), bk.detach().reshape(-1)])
        qk = gemm_bias_act(xd, w_qk, bias=b_qk, act=act)
        V = gemm_bias_act(xd, wv.detach(), out=gather_friendly_empty(n, U, wv.device))
        # K rows narrower than a 128-byte line are gathered per edge: inside [Q | K] a line holds half as many of them
        # (nn/conv/gat._project_qkv); a copy of [n, A] floats costs ~10 us
        K = qk[:, A:].contiguous() if A <= 16 else qk[:, A:]
        ctx.act, ctx.A, ctx.table = act, A, table
        ctx.save_for_backward(x, wq, wk, wv, bq, qk if act == L.ACT_RELU else None)
        return qk[:, :A], K, V

    @staticmethod
    def backward(ctx, gQ, gK, gV):
        x, wq, wk, wv, bq, qk = ctx.saved_tensors
        xd = _rows_of(x, ctx.table)
        A, U, n = ctx.A, int(wv.shape[1]), int(xd.shape[0])
        need = ctx.needs_input_grad
        D = torch.empty((n, 2 * A + U), dtype=torch.float32, device=wv.device)
        if ctx.act == L.ACT_RELU:
            relu_backward(gQ, qk[:, :A], into=D[:, :A])
            relu_backward(gK, qk[:, A:], into=D[:, A:2 * A])
        else:
            D[:, :A] = gQ
            D[:, A:2 * A] = gK
        D[:, 2 * A:] = gV
        gwq = gwk = gwv = gbq = gbk = gx = None
        if need[1] or need[2] or need[3] or need[4] or need[5]:
            gW, gb = gemm_tn(xd, D, want_bias=bq is not None and (need[2] or need[4]))
            gwq, gwk, gwv = gW[:, :A], gW[:, A:2 * A], gW[:, 2 * A:]
            if gb is not None:
                gbq, gbk = gb[:A], gb[A:2 * A]
        if need[0]:
            gx = gemm_bias_act(D, transpose(torch.cat([wq.detach(), wk.detach(), wv.detach()], dim=1)))
        return gx, gwq, gbq, gwk, gbk, gwv, None, None


def project_qkv(x, wq, bq, wk, bk, wv, act):
    """Differentiable (Q, K, V) of a GAT layer on dense features; Q and K share the (fused-code) activation `act`."""
    f = L.as_f32
    x, table = _gemm_source(x)
    return _ProjectQKV.apply(x, f(wq), None if bq is None else f(bq), f(wk), None if bk is None else f(bk), f(wv), act, table)


class _GatAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, num_heads, Q, K, V, drop_rate, drop_seed, scale_d=None, passes=None):
        """`passes` (the sharded path, dist/sharded.py::_gat_attention_spans): callable(Q, K, V, stats) -> out that runs the
        forward as span passes + merge under a halo exchange; same (out, stats), so the backward is unchanged."""
        from .nn.conv.gat import gat_attention, query_sums_apply, SOURCE_BLOCK_STATS
        stats = torch.empty((plan.n_dst, 2 * num_heads), dtype=torch.float32, device=V.device)
        ctx.halo_first = getattr(passes, "halo_first", None)   # (n_own, [(lo, hi) per round], callable(j, d[K | V])): see backward
        qsums = None
        if passes is not None:
            assert float(drop_rate) == 0.0 and scale_d is None
            out = passes(Q.detach(), K.detach(), V.detach(), stats)
        else:
            # one attention unit per head (the demo's literal layer): the walk also accumulates the two sums dQ is a per-row
            # expression of (tfgx_gat_args.qgrad_t) — the backward then runs no destination pass
            if ctx.needs_input_grad[2] and query_sums_apply(plan, Q, V, num_heads, float(drop_rate)):
                qsums = (torch.empty((plan.n_dst, int(V.shape[1])), dtype=torch.float32, device=V.device),
                         torch.empty((plan.n_dst, num_heads), dtype=torch.float32, device=V.device))
                SOURCE_BLOCK_STATS["query_sum_forwards"] = SOURCE_BLOCK_STATS.get("query_sum_forwards", 0) + 1
            out = gat_attention(plan, Q.detach(), K.detach(), V.detach(), num_heads, True, stats_ml=stats,
                                drop_rate=drop_rate, drop_seed=drop_seed, scale_d=scale_d, qsums=qsums)
        ctx.plan, ctx.H, ctx.drop = plan, num_heads, (float(drop_rate), drop_seed)      # (seed: host int or device tensor)
        ctx.scale_d = scale_d
        ctx.has_qsums = qsums is not None
        ctx.save_for_backward(Q, K, V, out, stats, *(qsums or ()))
        return out

    @staticmethod
    def backward(ctx, g):
        lib = L.require_gpu()
        plan, H = ctx.plan, ctx.H
        Q, K, V, out, stats = ctx.saved_tensors[:5]
        qsums = ctx.saved_tensors[5:7] if ctx.has_qsums else None
        Q2, ldq = L.row_major_2d(Q.detach())
        K2, ldk = L.row_major_2d(K.detach())
        V2, ldv = L.row_major_2d(V.detach())
        g2, ldg = L.row_major_2d(g.contiguous())
        n, A, W = plan.n_dst, int(Q2.shape[1]), int(V2.shape[1])
        # one sweep over the destination rows: D = <dO, O> per head AND the packed rows the source pass gathers — per
        # edge it needs the DESTINATION's dO, Q, (m, l) and D; interleaved into one row per destination, padded to whole
        # 128-byte lines, that is one burst of P*4 bytes per edge instead of four gathers (H=8, A=8, U=64: 96 floats =
        # 3 lines instead of 5).  Round 6: behind dO the row holds ONE block per head, [Q | m | 1 / (l + 1e-8) | D | pad] in
        # roundup4(d + 3) floats — every lane of a head then fetches its scalars with 16-byte loads of the same bytes: three
        # line REQUESTS per edge instead of five (tfgx_gat_backward_args.head_pack)
        HB = -(-(A // H + 3) // 4) * 4
        W4 = -(-W // 4) * 4                                      # the head blocks start on a 16-byte boundary of the row
        P = -(-(W4 + H * HB) // 32) * 32
        pack = torch.empty((n, P), dtype=torch.float32, device=g2.device)
        dsum = torch.empty((n, H), dtype=torch.float32, device=g2.device)
        out2, ldo = L.row_major_2d(out)
        L.check(lib.tfgx_gat_pack_dst_heads_f32(L.ptr(g2), ldg, L.ptr(out2), ldo, L.ptr(Q2), ldq, L.ptr(stats), n, H, A // H,
                                                W // H, L.ptr(pack), P, L.ptr(dsum), L.stream_ptr()),
                "tfgx_gat_pack_dst_heads_f32")
        pt, t2d = _transposed(plan)
        # dense outputs (K2 / V2 may be column slices of a wider table — the sharded [K | V] halo table)
        dev = g2.device
        gq = torch.empty((n, A), dtype=torch.float32, device=dev)
        hf = getattr(ctx, "halo_first", None)
        n_tab = int(K2.shape[0])
        if hf is not None and int(V2.shape[0]) == n_tab:
            # sharded [K | V] table: d[K | V] in ONE buffer (its halo rows travel back as one exchange), gk / gv are its column
            # blocks — what autograd's slice backward would assemble anyway
            gkv = torch.empty((n_tab, A + W), dtype=torch.float32, device=dev)
            gk, gv = gkv[:, :A], gkv[:, A:]
        else:
            hf, gkv = None, None
            gk = torch.empty((n_tab, A), dtype=torch.float32, device=dev)
            gv = torch.empty((int(V2.shape[0]), W), dtype=torch.float32, device=dev)
        a = L.GatBackwardArgs()
        a.row_ptr, a.col, a.n_dst = plan.row_ptr.data_ptr(), plan.col.data_ptr(), n
        a.row_ptr_t, a.dst_t, a.n_src = pt.row_ptr.data_ptr(), pt.col.data_ptr(), pt.n_dst
        a.q, a.ldq, a.k, a.ldk, a.v, a.ldv = Q2.data_ptr(), ldq, K2.data_ptr(), ldk, V2.data_ptr(), ldv
        a.grad_out, a.ld_grad_out = g2.data_ptr(), ldg
        a.stats_ml, a.dsum = stats.data_ptr(), dsum.data_ptr()
        a.H, a.d, a.dv, a.add_self_loop = H, A // H, W // H, 1
        a.scale = math.sqrt(float(A // H if ctx.scale_d is None else ctx.scale_d))
        a.grad_q, a.ld_grad_q = gq.data_ptr(), A
        a.grad_k, a.ld_grad_k = gk.data_ptr(), int(gk.stride(0))
        a.grad_v, a.ld_grad_v = gv.data_ptr(), int(gv.stride(0))
        ro, ro_t = plan.row_order(), pt.row_order()        # skewed graphs: degree-ordered walks (results unchanged)
        a.row_order = 0 if ro is None else ro.data_ptr()
        a.row_order_t = 0 if ro_t is None else ro_t.data_ptr()
        if ctx.drop[0] > 0.0:      # regenerate the forward's keep mask: same seed, forward-CSR edge positions
            from .nn.conv.gat import _set_drop
            _set_drop(a, ctx.drop[0], ctx.drop[1], plan.num_edges)
            a.edge_pos_t = t2d.data_ptr()
        # power-law graphs: rows too long for one lane group are walked chunk-wise (the plans' hub lists) and their chunk
        # partials added in order — dQ over the forward plan's hub destinations, dK / dV over the transposed plan's hub sources
        hub_d, nc_d = L.hub_lists(plan)
        sc_d = torch.empty(max(nc_d * A, 1), dtype=torch.float32, device=dev) if hub_d is not None else None
        # dense graphs: both passes in chained launches over the blocks of the OTHER endpoint (nn/conv/gat.source_block_count:
        # each launch gathers rows of one block, served by the L2 of every XCD; gradients accumulate block by block)
        from .nn.conv.gat import source_block_count, SOURCE_BLOCK_STATS
        from .nn.conv import gat as G_
        d_h, dv_h = A // H, W // H
        blocks_ok = (ctx.drop[0] <= 0.0 and hf is None and hub_d is None and ro is None and ro_t is None and
                     d_h in (1, 2, 4, 8, 16, 32) and dv_h % 4 == 0 and dv_h // 4 <= 64 and
                     (((dv_h // 4) & (dv_h // 4 - 1)) == 0 or H == 1) and ldv % 4 == 0 and ldg % 4 == 0 and
                     V2.data_ptr() % 16 == 0 and g2.data_ptr() % 16 == 0)
        kb_d = source_block_count(plan, A, W) if blocks_ok else 1
        blk_d = plan.source_blocks(kb_d) if kb_d >= 2 else None
        if qsums is not None:
            # dQ from the forward's sums: (<dO, T> - D S) / scale per (row, head) — no walk over the edges
            L.check(lib.tfgx_gat_query_grad_d1_f32(L.ptr(g2), ldg, L.ptr(qsums[0]), W, L.ptr(qsums[1]), L.ptr(dsum), n, H, W // H,
                                                   a.scale, L.ptr(gq), A, L.stream_ptr()), "tfgx_gat_query_grad_d1_f32")
            SOURCE_BLOCK_STATS["query_sum_backwards"] = SOURCE_BLOCK_STATS.get("query_sum_backwards", 0) + 1
        elif blk_d is not None:
            rpk, col_k = blk_d
            for b in range(kb_d):
                a.col = col_k.data_ptr()
                a.span_begin, a.span_end, a.span_stride = rpk[b:].data_ptr(), rpk[b + 1:].data_ptr(), kb_d
                a.accumulate, a.add_self_loop = (1 if b else 0), (1 if b == kb_d - 1 else 0)
                L.check(lib.tfgx_gat_backward_dst_hub_f32(ctypes.byref(a), None, None, L.stream_ptr()),
                        "tfgx_gat_backward_dst_hub_f32 (source block)")
            a.col, a.span_begin, a.span_end, a.span_stride, a.accumulate, a.add_self_loop = plan.col.data_ptr(), 0, 0, 0, 0, 1
            SOURCE_BLOCK_STATS["backward_launches"] = SOURCE_BLOCK_STATS.get("backward_launches", 0) + kb_d
        else:
            L.check(lib.tfgx_gat_backward_dst_hub_f32(ctypes.byref(a), None if hub_d is None else ctypes.byref(hub_d),
                                                      L.ptr(sc_d), L.stream_ptr()), "tfgx_gat_backward_dst_hub_f32")
        a.grad_out, a.ld_grad_out = pack.data_ptr(), P            # dO out of the packed rows; Q / (m, l) / D stay the dense arrays
        a.head_pack, a.ld_head_pack = pack.data_ptr() + 4 * W4, P  # (read by the one-lane kernels of odd head geometries only)
        hub_s, nc_s = L.hub_lists(pt)
        sc_s = torch.empty(max(nc_s * (A + W), 1), dtype=torch.float32, device=dev) if hub_s is not None else None
        if hf is not None and hub_s is None and 0 < hf[0] < n_tab:
            # halo rows of the table first (sources that are no destinations: no self-loop, window-relative row indices:
            # the K / V / gradient pointers move with the window), their gradients start travelling, then the own rows
            n_own = int(hf[0])
            full = (a.row_ptr_t, a.n_src, a.k, a.v, a.grad_k, a.grad_v, a.add_self_loop, a.row_order_t)
            a.add_self_loop, a.row_order_t = 0, 0
            for j, (lo, hi) in enumerate(hf[1]):               # one window per exchange round (the halo rows are round-major)
                if hi > lo:
                    a.row_ptr_t = pt.row_ptr.data_ptr() + 4 * lo
                    a.n_src = hi - lo
                    a.k, a.v = K2.data_ptr() + 4 * ldk * lo, V2.data_ptr() + 4 * ldv * lo
                    a.grad_k = gk.data_ptr() + 4 * int(gk.stride(0)) * lo
                    a.grad_v = gv.data_ptr() + 4 * int(gv.stride(0)) * lo
                    L.check(lib.tfgx_gat_backward_src_hub_f32(ctypes.byref(a), None, None, L.stream_ptr()),
                            "tfgx_gat_backward_src_hub_f32 (halo rows)")
                hf[2](j, gkv)
            a.row_ptr_t, a.n_src, a.k, a.v, a.grad_k, a.grad_v, a.add_self_loop, a.row_order_t = full
            a.n_src, a.row_order_t = n_own, 0
            L.check(lib.tfgx_gat_backward_src_hub_f32(ctypes.byref(a), None, None, L.stream_ptr()),
                    "tfgx_gat_backward_src_hub_f32 (own rows)")
        else:
            # the source pass gathers the packed DESTINATION rows (P floats each): blocks of destinations
            kb_s = source_block_count(pt, P, 0) if (blocks_ok and hub_s is None and gv.stride(0) % 4 == 0) else 1
            if kb_s >= 2 and G_.DESTINATION_BLOCKS is not None:
                kb_s = max(int(G_.DESTINATION_BLOCKS), 1)       # developer A/B (tools/r06/sweep_gat_bwd_blocks.py)
            blk_s = pt.source_blocks(kb_s) if kb_s >= 2 else None
            if blk_s is not None:
                rpk_t, dst_k = blk_s
                for b in range(kb_s):
                    a.dst_t = dst_k.data_ptr()
                    a.span_begin, a.span_end, a.span_stride = rpk_t[b:].data_ptr(), rpk_t[b + 1:].data_ptr(), kb_s
                    a.accumulate, a.add_self_loop = (1 if b else 0), (1 if b == kb_s - 1 else 0)
                    L.check(lib.tfgx_gat_backward_src_hub_f32(ctypes.byref(a), None, None, L.stream_ptr()),
                            "tfgx_gat_backward_src_hub_f32 (destination block)")
                SOURCE_BLOCK_STATS["backward_launches"] = SOURCE_BLOCK_STATS.get("backward_launches", 0) + kb_s
            else:
                L.check(lib.tfgx_gat_backward_src_hub_f32(ctypes.byref(a), None if hub_s is None else ctypes.byref(hub_s),
                                                          L.ptr(sc_s), L.stream_ptr()), "tfgx_gat_backward_src_hub_f32")
        return None, None, gq, gk, gv, None, None, None, None


def gat_attention(plan, Q, K, V, num_heads, drop_rate=0.0, drop_seed=0, scale_d=None, passes=None):
    """Differentiable fused attention (self-loop edge appended, as nn/conv/gat.py:43); drop_rate > 0 = training-time
    dropout of the attention weights (gat.py:85).  scale_d: the per-head width the scores are scaled by when Q / K
    arrive zero-padded per head (nn/conv/gat._kernel_widths)."""
    return _GatAttention.apply(plan, num_heads, Q, K, V, float(drop_rate),
                               drop_seed if isinstance(drop_seed, torch.Tensor) else int(drop_seed), scale_d, passes)


def edge_attr_csr(plan, edge_attr, cache=None):
    """edge attribute (caller's edge order) -> the plan's CSR order; a differentiable permutation when the attribute is
    being tracked, the memoised kernel copy (plan.edge_weight_csr) otherwise."""
    from .plan import edge_weight_csr
    if edge_attr is None:
        return None
    if needs_grad(edge_attr):
        return L.as_f32(edge_attr)[plan.perm.long()]
    return edge_weight_csr(plan, edge_attr, cache)


def gather(x, idx):
    """x[idx] (tf.gather): the gather kernel, or torch indexing when x is being tracked."""
    from .plan import gather_rows
    if needs_grad(x):
        return L.as_f32(x)[L.as_i32(idx).long()]
    return gather_rows(x, idx)


class _SegmentSoftmax(torch.autograd.Function):
    """out = exp(d - stop_gradient(segmax)) / (segsum + 1e-8)  (nn/kernel/segment.py:26-33):
    d out_i / d d_j = [i == j] out_i - out_i out_j inside a segment, so grad = out * (g - segsum(out * g))."""

    @staticmethod
    def forward(ctx, plan, ids, d):
        lib = L.require_gpu()
        dd = d.detach().contiguous()
        out = torch.empty_like(dd)
        H = 1 if dd.dim() == 1 else int(dd.shape[1])
        if int(ids.shape[0]):
            L.edge_softmax(plan, dd, H, out)
        ctx.plan, ctx.ids = plan, ids
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        s = out * g
        s2 = s if s.dim() == 2 else s.unsqueeze(1)
        # plan.col is all zeros for this plan: reduce the E explicit rows through perm instead
        seg = segment_reduce(ctx.plan, s2.contiguous(), L.SUM, col=ctx.plan.perm)
        back = seg[ctx.ids.long()]
        return None, None, s - out * (back if s.dim() == 2 else back[:, 0])


def segment_softmax(plan, ids, data):
    return _SegmentSoftmax.apply(plan, ids, data)


class _BiasAdd(torch.autograd.Function):
    """h + bias (broadcast over rows).  torch's own add would do — but its backward reduces the [N, units] gradient with
    g.sum(0), which runs odd widths (47 classes of ogbn-products, 41 of Reddit) at 24 GB/s: 19 ms per step at products shape.
    The backward here is the two-phase column-sum kernel (plan.column_sums)."""

    @staticmethod
    def forward(ctx, h, bias):
        return h + bias

    @staticmethod
    def backward(ctx, g):
        return (g if ctx.needs_input_grad[0] else None), (column_sums(g) if ctx.needs_input_grad[1] else None)


def bias_add(h, bias):
    """h + bias for a [N, units] activation and a [units] bias (differentiable; None bias: h itself)."""
    if bias is None:
        return h
    b = L.as_f32(bias)
    if h.dim() == 2 and b.dim() == 1 and h.is_cuda and needs_grad(b):
        return _BiasAdd.apply(h, b)
    return h + b


def apply_activation(h, act, post):
    if act == L.ACT_RELU:
        h = torch.relu(h)
    return post(h) if post is not None else h


class _GatherScale(torch.autograd.Function):
    """out[i, :] = x[idx[i], :] * s[idx[i]] (SAGPool: (x * score)[kept]; s = None: SortPool's plain gather).
    Forward = tfgx_gather_scale_rows_f32; backward = tfgx_gather_scale_rows_backward_f32, one launch over every parent row
    through node_map (dropped rows get 0): dx = g[node_map] * s, ds = sum_f g[node_map] * x (fixed-order wave sum)."""

    @staticmethod
    def forward(ctx, x, s, idx, node_map):
        lib = L.require_gpu()
        x2, ldx = L.row_major_2d(x)
        M, F = int(idx.shape[0]), int(x2.shape[1])
        out = torch.empty((M, F), dtype=torch.float32, device=x2.device)
        L.check(lib.tfgx_gather_scale_rows_f32(L.ptr(x2), ldx, L.ptr(idx), L.ptr(s), M, F, L.ptr(out), max(F, 1),
                                               L.stream_ptr()), "tfgx_gather_scale_rows_f32")
        ctx.save_for_backward(x2, s, node_map)
        ctx.has_s = s is not None
        return out

    @staticmethod
    def backward(ctx, g):
        lib = L.require_gpu()
        x2, s, node_map = ctx.saved_tensors
        need_x = ctx.needs_input_grad[0]
        need_s = ctx.has_s and ctx.needs_input_grad[1]
        n, F = int(x2.shape[0]), int(x2.shape[1])
        g2, ldg = L.row_major_2d(g.to(torch.float32))
        dx = torch.empty((n, F), dtype=torch.float32, device=x2.device) if need_x else None
        ds = torch.empty(n, dtype=torch.float32, device=x2.device) if need_s else None
        ldx = x2.stride(0) if n > 1 else max(F, 1)
        L.check(lib.tfgx_gather_scale_rows_backward_f32(L.ptr(g2), ldg, L.ptr(node_map), n, L.ptr(x2), ldx, L.ptr(s), F,
                                                        L.ptr(dx), max(F, 1), L.ptr(ds), L.stream_ptr()),
                "tfgx_gather_scale_rows_backward_f32")
        return dx, ds, None, None


def gather_scale(x, idx, node_map, s=None):
    """(x * s[:, None])[idx] with s = a per-node multiplier ([n] or [n, 1]) or None; node_map[v] = position of v in idx
    or -1 (tfgx_induced_subgraph_count).  Differentiable wrt x and s."""
    n = int(x.shape[0])
    if s is not None:
        s = L.as_f32(s, x.device)
        if s.numel() != n:
            raise ValueError("the node score must hold one value per node ([{0}] or [{0}, 1]), got shape {1}".format(
                n, tuple(s.shape)))
        s = s.reshape(-1)
        if not s.is_contiguous():
            s = s.contiguous()
    return _GatherScale.apply(x, s, L.as_i32(idx, x.device), node_map)


class _GatherScaleStatic(torch.autograd.Function):
    """_GatherScale at a fixed shape (nn.sag_pool_static): idx holds -1 for the dead pooled rows, which come out exactly 0
    (tfgx_static_pool_gather_scale_rows_f32: a clamped load, then a select).  The backward is _GatherScale's."""

    @staticmethod
    def forward(ctx, x, s, idx, node_map):
        lib = L.require_gpu()
        x2, ldx = L.row_major_2d(x)
        M, F = int(idx.shape[0]), int(x2.shape[1])
        out = torch.empty((M, F), dtype=torch.float32, device=x2.device)
        L.check(lib.tfgx_static_pool_gather_scale_rows_f32(L.ptr(x2), ldx, int(x2.shape[0]), L.ptr(idx), L.ptr(s), M, F, L.ptr(out),
                                                           max(F, 1), L.stream_ptr()), "tfgx_static_pool_gather_scale_rows_f32")
        ctx.save_for_backward(x2, s, node_map)
        ctx.has_s = s is not None
        return out

    backward = staticmethod(_GatherScale.backward)


def gather_scale_static(x, idx, node_map, s=None):
    """gather_scale for a pooled static batch: idx int32 [n_cap'] with -1 for dead rows (zero rows of the result), node_map
    int32 [n_cap].  Differentiable wrt x and s."""
    n = int(x.shape[0])
    if s is not None:
        s = L.as_f32(s, x.device)
        if s.numel() != n:
            raise ValueError("the node score must hold one value per node ([{0}] or [{0}, 1]), got shape {1}".format(
                n, tuple(s.shape)))
        s = s.reshape(-1)
        if not s.is_contiguous():
            s = s.contiguous()
    return _GatherScaleStatic.apply(x, s, idx, node_map)


class _SegmentRows3D(torch.autograd.Function):
    """Node rows -> the [G * k, F] rows of the dense [G, k, F] tensor (tfgx_segment_rows_3d_f32, one launch): the plain mode
    (sort_col None: convert_x_to_3d) or the sort mode (SortPool's ranking by column sort_col of x).  Returns (out, slot_node,
    flags).  The backward is one gather through node_slot (tfgx_static_pool_gather_scale_rows_f32 without a multiplier): every
    row of dx is written once, as a copy or as zeros."""

    @staticmethod
    def forward(ctx, x, seg_ptr, seg_node, G, N, k, sort_col):
        lib = L.require_gpu()
        x2, ldx = L.row_major_2d(x)
        n_rows, F = int(x2.shape[0]), int(x2.shape[1])
        dev = x2.device
        out = torch.empty((G * k, F), dtype=torch.float32, device=dev)
        slot_node = torch.empty(G * k, dtype=torch.int32, device=dev)
        node_slot = torch.empty(n_rows, dtype=torch.int32, device=dev)
        flags = torch.empty(1, dtype=torch.int32, device=dev)
        key = None if sort_col is None else ctypes.c_void_p(x2.data_ptr() + 4 * int(sort_col))
        L.check(lib.tfgx_segment_rows_3d_f32(L.ptr(seg_ptr), L.ptr(seg_node), G, N, L.ptr(x2), ldx, n_rows, F, k, key, ldx,
                                             L.ptr(out), max(F, 1), L.ptr(slot_node), L.ptr(node_slot), L.ptr(flags),
                                             L.stream_ptr()), "tfgx_segment_rows_3d_f32")
        ctx.save_for_backward(node_slot)
        ctx.slots, ctx.F = G * k, F
        ctx.mark_non_differentiable(slot_node, flags)
        return out, slot_node, flags

    @staticmethod
    def backward(ctx, g, _slot_node, _flags):
        lib = L.require_gpu()
        node_slot, = ctx.saved_tensors
        n_rows, F = int(node_slot.shape[0]), ctx.F
        if ctx.slots == 0 or n_rows == 0 or F == 0:
            return (torch.zeros((n_rows, F), dtype=torch.float32, device=node_slot.device),) + (None,) * 6
        g2, ldg = L.row_major_2d(g.to(torch.float32))
        dx = torch.empty((n_rows, F), dtype=torch.float32, device=g2.device)
        L.check(lib.tfgx_static_pool_gather_scale_rows_f32(L.ptr(g2), ldg, ctx.slots, L.ptr(node_slot), None, n_rows, F, L.ptr(dx),
                                                           F, L.stream_ptr()), "tfgx_static_pool_gather_scale_rows_f32")
        return (dx,) + (None,) * 6


def segment_rows_3d(x, seg_ptr, seg_node, G, N, k, sort_col=None):
    """(out [G * k, F], slot_node int32 [G * k], flags int32 [1]) of tfgx_segment_rows_3d_f32 over the graph plan (seg_ptr
    int32 [G + 1], seg_node int32 [N] or None = the identity); differentiable wrt x.  sort_col: a column of x in [0, F)."""
    return _SegmentRows3D.apply(x, seg_ptr, seg_node, int(G), int(N), int(k), sort_col)


def gather_edge_values(w, edge_id):
    """w[edge_id] for a 1-D float32 tensor (tfgx_permute_rows_f32 with width 1)."""
    lib = L.require_gpu()
    w = w.contiguous()
    out = torch.empty(int(edge_id.shape[0]), dtype=torch.float32, device=w.device)
    if int(edge_id.shape[0]):
        L.check(lib.tfgx_permute_rows_f32(L.ptr(w), L.ptr(edge_id), int(edge_id.shape[0]), 1, L.ptr(out), L.stream_ptr()),
                "tfgx_permute_rows_f32")
    return out


class _GatherEdges(torch.autograd.Function):
    """w[edge_id] for a tracked 1-D edge attribute; edge ids are unique, so the backward is a plain scatter into zeros
    (tfgx_scatter_add_rows_f32 on a zeroed buffer: no conflicts, deterministic)."""

    @staticmethod
    def forward(ctx, w, edge_id):
        ctx.save_for_backward(edge_id)
        ctx.E = int(w.shape[0])
        return gather_edge_values(w, edge_id)

    @staticmethod
    def backward(ctx, g):
        lib = L.require_gpu()
        (edge_id,) = ctx.saved_tensors
        dw = torch.zeros(ctx.E, dtype=torch.float32, device=g.device)
        gc = g.to(torch.float32).contiguous()
        if int(edge_id.shape[0]):
            L.check(lib.tfgx_scatter_add_rows_f32(L.ptr(dw), 1, L.ptr(edge_id), int(edge_id.shape[0]), 1, L.ptr(gc), 1,
                                                  L.stream_ptr()), "tfgx_scatter_add_rows_f32")
        return dw, None


def gather_edges(w, edge_id):
    return _GatherEdges.apply(L.as_f32(w).reshape(-1), edge_id)


def edge_dot_forward(z, z_other, row, col, bad_flag=None):
    """One tfgx_edge_dot_f32 launch (include/tfgx_linkpred.h): out[e] = <z[row[e]], z_other[col[e]]>, no plan."""
    lib = L.require_gpu()
    a, lda = L.row_major_2d(z)
    b, ldb = (a, lda) if z_other is z else L.row_major_2d(z_other)
    E = int(row.shape[0])
    out = torch.empty(E, dtype=torch.float32, device=a.device)
    L.check(lib.tfgx_edge_dot_f32(L.ptr(row), L.ptr(col), E, L.ptr(a), lda, int(a.shape[0]), L.ptr(b), ldb, int(b.shape[0]),
                                  int(a.shape[1]), L.ptr(out), L.ptr(bad_flag), L.stream_ptr()), "tfgx_edge_dot_f32")
    return out


class _EdgeDot(torch.autograd.Function):
    """logit[e] = <z[row[e]], z_other[col[e]]> (the link-prediction decoder).  Backward on the aggregation kernels:
    dz[i] = sum_{e: row[e] = i} g[e] * z_other[col[e]] is a weighted segment sum on the list's plan, d z_other the same on
    the transposed plan; with a shared table (z_other is None) the two are added.  Fixed reduction order: bit-reproducible."""

    @staticmethod
    def forward(ctx, plan, z, z_other, row, col):
        ctx.plan = plan
        zd = z.detach()
        ctx.save_for_backward(z, z_other)
        return edge_dot_forward(zd, zd if z_other is None else z_other.detach(), row, col)

    @staticmethod
    def backward(ctx, g):
        plan = ctx.plan
        z, z_other = ctx.saved_tensors
        shared = z_other is None
        other = z if shared else z_other
        g = g.contiguous()
        gz = go = None
        if ctx.needs_input_grad[1]:
            gz = segment_reduce(plan, other.detach(), L.SUM, w_csr=plan.edge_attr_to_csr(g))
        if shared or ctx.needs_input_grad[2]:
            pt = plan.transposed()
            go = segment_reduce(pt, z.detach(), L.SUM, w_csr=pt.edge_attr_to_csr(g))
        if shared:
            return None, (gz + go) if gz is not None else None, None, None, None
        return None, gz, go if ctx.needs_input_grad[2] else None, None, None


def edge_dot(plan, z, z_other, row, col):
    return _EdgeDot.apply(plan, z, z_other, row, col)


# ---- the LSTM aggregator of GraphSAGE (include/tfgx_lstm.h)
def lstm_max_degree(plan):
    """T of the LSTM aggregator: the plan's longest row, read once (the layer's only host synchronisation) and kept on the plan."""
    if getattr(plan, "_max_degree", None) is None:
        plan._max_degree = int(plan.in_degree().max().item()) if (plan.n_dst > 0 and plan.num_edges > 0) else 0
    return plan._max_degree


def _lstm_step_plan(plan, T):
    """The plan of dP[j] = sum over (i, t) with neighbour j of d_gates[i * T + t]: the transposed plan's rows with the column
    of an edge replaced by i * T + its position t inside row i of `plan`.  Derived once per (plan, T), kept on the plan."""
    memo = getattr(plan, "_lstm_step_plans", None)
    if memo is None:
        memo = plan._lstm_step_plans = {}
    if T not in memo:
        if plan.n_dst * T >= (1 << 31):
            raise L.TfgxError("lstm_aggregate: n_dst * T = {} does not fit the int32 columns of a plan".format(plan.n_dst * T))
        pt, t2d = _transposed(plan)
        dst = pt.col.long()
        step = t2d.long() - plan.row_ptr.long()[dst]
        from .plan import CsrPlan
        memo[T] = CsrPlan(pt.row_ptr, (dst * T + step).to(torch.int32).contiguous(), pt.perm, pt.n_dst, plan.n_dst * T,
                          pt.num_edges)
    return memo[T]


def lstm_aggregate_forward(plan, T, P, p_pad, R, saved=None, bad_flag=None):
    """One launch of tfgx_lstm_aggregate_f32: [plan.n_dst, U] mean of h_t over the T steps of every row."""
    lib = L.require_gpu()
    P, ldp = L.row_major_2d(P)
    R = R.contiguous()
    U = int(R.shape[0])
    out = torch.empty((plan.n_dst, U), dtype=torch.float32, device=P.device)
    L.check(lib.tfgx_lstm_aggregate_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), plan.n_dst, plan.n_src, T, L.ptr(P), ldp,
                                        L.ptr(p_pad.contiguous()), L.ptr(R), U, L.ptr(out), U, L.ptr(saved),
                                        0 if saved is None else int(saved.numel()), L.ptr(bad_flag), L.stream_ptr()),
            "tfgx_lstm_aggregate_f32")
    return out


class _LstmAggregate(torch.autograd.Function):
    """mean_t h_t of the unmasked LSTM over every row's padded neighbour sequence, inputs (P, p_pad, R) (tfgx_lstm.h)."""

    @staticmethod
    def forward(ctx, plan, T, P, p_pad, R):
        lib = L.require_gpu()
        U = int(R.shape[0])
        saved = torch.empty(max(lib.tfgx_lstm_aggregate_saved_bytes(plan.n_dst, T, U), 1), dtype=torch.uint8, device=P.device)
        out = lstm_aggregate_forward(plan, T, P.detach(), p_pad.detach(), R.detach(), saved=saved)
        ctx.plan, ctx.T, ctx.n_src = plan, T, int(P.shape[0])
        ctx.save_for_backward(R, saved)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = L.require_gpu()
        plan, T = ctx.plan, ctx.T
        R, saved = ctx.saved_tensors
        R = R.detach().contiguous()
        U = int(R.shape[0])
        g, ldd = L.row_major_2d(g)
        dev = g.device
        if plan.n_dst == 0 or T == 0:
            return (None, None, torch.zeros((ctx.n_src, 4 * U), dtype=torch.float32, device=dev),
                    torch.zeros(4 * U, dtype=torch.float32, device=dev), torch.zeros_like(R))
        d_gates = torch.empty((plan.n_dst * T, 4 * U), dtype=torch.float32, device=dev)
        h_prev = torch.empty((plan.n_dst * T, U), dtype=torch.float32, device=dev)
        d_pad = torch.empty((lib.tfgx_lstm_aggregate_tiles(plan.n_dst), 4 * U), dtype=torch.float32, device=dev)
        L.check(lib.tfgx_lstm_aggregate_backward_f32(L.ptr(plan.row_ptr), plan.n_dst, T, U, L.ptr(R), L.ptr(g), ldd, L.ptr(saved),
                                                     int(saved.numel()), L.ptr(d_gates), L.ptr(h_prev), L.ptr(d_pad),
                                                     L.stream_ptr()), "tfgx_lstm_aggregate_backward_f32")
        gP = gpad = gR = None
        if ctx.needs_input_grad[2]:
            if plan.num_edges > 0:
                gP = segment_reduce(_lstm_step_plan(plan, T), d_gates, L.SUM)
            else:
                gP = torch.zeros((ctx.n_src, 4 * U), dtype=torch.float32, device=dev)
        if ctx.needs_input_grad[3]:
            gpad = column_sums(d_pad)
        if ctx.needs_input_grad[4]:
            gR = gemm_tn(h_prev, d_gates)[0]
        return None, None, gP, gpad, gR


def lstm_aggregate(plan, T, P, p_pad, R):
    """[plan.n_dst, U]: the LSTM aggregator's neighbour term before neighbor_kernel.  P [plan.n_src, 4U] = x @ kernel + bias,
    p_pad [4U] = the projection of a zero row, R [U, 4U]; U a multiple of 16 up to 256.  Differentiable in P, p_pad and R."""
    if needs_grad(P, p_pad, R):
        return _LstmAggregate.apply(plan, T, P, p_pad, R)
    return lstm_aggregate_forward(plan, T, P, p_pad, R)


# ---- Set2Set (include/tfgx_set2set.h): the stateful sequence LSTM and the per-graph attention readout
def lstm_sequence_forward(P, B, T, R, h0=None, c0=None, saved=None):
    """One launch of tfgx_lstm_sequence_f32 over P [B * T, 4U]: (h_seq [B * T, U], h_last [B, U], c_last [B, U])."""
    lib = L.require_gpu()
    P, ldp = L.row_major_2d(P)
    R = R.contiguous()
    U = int(R.shape[0])
    dev = P.device
    h_seq = torch.empty((B * T, U), dtype=torch.float32, device=dev)
    h_last = torch.empty((B, U), dtype=torch.float32, device=dev)
    c_last = torch.empty((B, U), dtype=torch.float32, device=dev)
    L.check(lib.tfgx_lstm_sequence_f32(L.ptr(P), ldp, B, T, L.ptr(R), U, L.ptr(h0), L.ptr(c0), L.ptr(h_seq), L.ptr(h_last),
                                       L.ptr(c_last), L.ptr(saved), 0 if saved is None else int(saved.numel()), L.stream_ptr()),
            "tfgx_lstm_sequence_f32")
    return h_seq, h_last, c_last


class _LstmSequence(torch.autograd.Function):
    """(h_seq, h_last, c_last) of an LSTM over B sequences of T steps with the input projection P hoisted and an initial
    state (h0, c0) (tfgx_set2set.h).  dP is the kernel's d_gates itself, dR = h_prev^T @ d_gates on the gemm_tn kernel."""

    @staticmethod
    def forward(ctx, P, B, T, R, h0, c0):
        lib = L.require_gpu()
        U = int(R.shape[0])
        h0d, c0d = h0.detach().contiguous(), c0.detach().contiguous()
        saved = torch.empty(max(lib.tfgx_lstm_sequence_saved_bytes(B, T, U), 1), dtype=torch.uint8, device=P.device)
        out = lstm_sequence_forward(P.detach(), B, T, R.detach(), h0d, c0d, saved=saved)
        ctx.B, ctx.T = B, T
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(R, h0d, saved)
        return out

    @staticmethod
    def backward(ctx, g_seq, g_h, g_c):
        lib = L.require_gpu()
        B, T = ctx.B, ctx.T
        R, h0, saved = ctx.saved_tensors
        R = R.detach().contiguous()
        U = int(R.shape[0])
        dev = R.device
        g_seq, g_h, g_c = (None if g is None else g.to(torch.float32).contiguous() for g in (g_seq, g_h, g_c))
        d_gates = torch.empty((B * T, 4 * U), dtype=torch.float32, device=dev)
        h_prev = torch.empty((B * T, U), dtype=torch.float32, device=dev)
        d_h0 = torch.empty((B, U), dtype=torch.float32, device=dev)
        d_c0 = torch.empty((B, U), dtype=torch.float32, device=dev)
        L.check(lib.tfgx_lstm_sequence_backward_f32(B, T, U, L.ptr(R), L.ptr(h0), L.ptr(g_seq), L.ptr(g_h), L.ptr(g_c),
                                                    L.ptr(saved), int(saved.numel()), L.ptr(d_gates), L.ptr(h_prev),
                                                    L.ptr(d_h0), L.ptr(d_c0), L.stream_ptr()), "tfgx_lstm_sequence_backward_f32")
        need = ctx.needs_input_grad
        gR = gemm_tn(h_prev, d_gates)[0] if need[3] else None
        return (d_gates if need[0] else None), None, None, gR, (d_h0 if need[4] else None), (d_c0 if need[5] else None)


def lstm_sequence(P, B, T, R, h0, c0):
    """(h_seq [B * T, U], h_last, c_last [B, U]); P [B * T, 4U] (row b * T + t), R [U, 4U], h0 / c0 [B, U]; U a multiple of 16
    up to 256, B * T > 0.  Differentiable in P, R, h0 and c0."""
    if needs_grad(P, R, h0, c0):
        return _LstmSequence.apply(P, B, T, R, h0, c0)
    return lstm_sequence_forward(P, B, T, R, h0.contiguous(), c0.contiguous())


def set2set_attend_forward(plan, x, q, stats=None, bad_flag=None):
    """One tfgx_set2set_attend_f32 call on a graph plan (rows = graphs, col = node ids): r [G, F]."""
    lib = L.require_gpu()
    x, ldx = L.row_major_2d(x)
    q, ldq = L.row_major_2d(q)
    G, N, F = plan.n_dst, int(x.shape[0]), int(x.shape[1])
    r = torch.empty((G, F), dtype=torch.float32, device=x.device)
    ws_bytes = lib.tfgx_set2set_attend_workspace_bytes(N, G, F)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    L.check(lib.tfgx_set2set_attend_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), G, N, L.ptr(x), ldx, F, L.ptr(q), ldq, L.ptr(r),
                                        max(F, 1), L.ptr(stats), L.ptr(ws), ws_bytes, L.ptr(bad_flag), L.stream_ptr()),
            "tfgx_set2set_attend_f32")
    return r


class _Set2SetAttend(torch.autograd.Function):
    """r_g = sum_n softmax_g(<x_n, q_g>) x_n with the reference's epsilon (segment.py:26-33): one pass over x forward, one
    pass backward (tfgx_set2set.h).  The statistics (m, D) are kept only here, where gradients are recorded."""

    @staticmethod
    def forward(ctx, plan, x, q):
        xd, qd = x.detach(), q.detach()
        stats = torch.empty((plan.n_dst, 2), dtype=torch.float32, device=xd.device)
        r = set2set_attend_forward(plan, xd, qd, stats=stats)
        ctx.plan = plan
        ctx.save_for_backward(xd, qd, r, stats)
        return r

    @staticmethod
    def backward(ctx, g):
        lib = L.require_gpu()
        plan = ctx.plan
        x, q, r, stats = ctx.saved_tensors
        x, ldx = L.row_major_2d(x)
        q, ldq = L.row_major_2d(q)
        g, ldg = L.row_major_2d(g.to(torch.float32))
        G, N, F = plan.n_dst, int(x.shape[0]), int(x.shape[1])
        d_x = None
        if ctx.needs_input_grad[1]:
            # every row has exactly one writer when the plan names every node; rows it skips must read as zero
            d_x = (torch.empty if plan.num_edges == N else torch.zeros)((N, F), dtype=torch.float32, device=x.device)
        d_q = torch.empty((G, F), dtype=torch.float32, device=x.device)
        ws_bytes = lib.tfgx_set2set_attend_workspace_bytes(N, G, F)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
        L.check(lib.tfgx_set2set_attend_backward_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), G, N, L.ptr(x), ldx, F, L.ptr(q), ldq,
                                                     L.ptr(r), max(F, 1), L.ptr(stats), L.ptr(g), ldg, L.ptr(d_x), max(F, 1),
                                                     L.ptr(d_q), max(F, 1), L.ptr(ws), ws_bytes, L.stream_ptr()),
                "tfgx_set2set_attend_backward_f32")
        return None, d_x, (d_q if ctx.needs_input_grad[2] else None)


def set2set_attend(plan, x, q):
    """[G, F] attention readout of x [N, F] under the queries q [G, F]; plan = the graph plan of node_graph_index."""
    if needs_grad(x, q):
        return _Set2SetAttend.apply(plan, x, q)
    return set2set_attend_forward(plan, x, q)


def dropout_keep_scale(seed, positions, rate):
    """tfgx_dropout_keep(seed, position, rate) / (1 - rate) for an int64 tensor of positions, as torch integer arithmetic on
    the device (csrc/tfgx_common.h drop_hash: murmur3's finaliser over position ^ seed_lo, seed_hi mixed in between the two
    multiplies; keep <=> top 24 bits >= rate * 2^24).  The statement of the in-kernel mask for the composed routes."""
    import numpy as np
    m = 0xFFFFFFFF
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    v = (positions.to(torch.int64) & m) ^ (seed & m)
    v = v ^ (v >> 16)
    v = (v * 0x85ebca6b) & m
    v = v ^ (seed >> 32)
    v = v ^ (v >> 13)
    v = (v * 0xc2b2ae35) & m
    v = v ^ (v >> 16)
    thr = int(np.float32(rate) * np.float32(16777216.0))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))
    return ((v >> 8) >= thr).to(torch.float32) * scale


def plan_rows(plan):
    """int64 [E]: the destination row of every CSR position (no host read: the output size is the plan's edge count)."""
    if getattr(plan, "_rows64", None) is None:
        ar = torch.arange(plan.n_dst, dtype=torch.int64, device=plan.col.device)
        plan._rows64 = torch.repeat_interleave(ar, plan.in_degree().to(torch.int64), output_size=plan.num_edges)
    return plan._rows64


def asap_attend_forward(plan, x, sq, sh, bias, drop_rate=0.0, seed=0, bad_flag=None, skip_self_loops=False):
    """One tfgx_asap_attend_f32 call on a square plan: (c [N, F], p [E], p_self [N], p_drop, p_self_drop) — the last two are
    None without dropout (they would equal p and p_self).  skip_self_loops, or a seed that is a device tensor (int64 [1]:
    nn.conv.gat.new_drop_seed inside a capture), takes tfgx_asapstatic_attend_f32 — the same kernel body with edges row == col
    absent and the seed read from device memory."""
    lib = L.require_gpu()
    x, ldx = L.row_major_2d(x)
    N, E, F = plan.n_dst, plan.num_edges, int(x.shape[1])
    dev = x.device
    c = torch.empty((N, F), dtype=torch.float32, device=dev)
    p = torch.empty(E, dtype=torch.float32, device=dev)
    p_self = torch.empty(N, dtype=torch.float32, device=dev)
    pd = pds = None
    if drop_rate > 0.0:
        pd, pds = torch.empty_like(p), torch.empty_like(p_self)
    seed_dev = seed if isinstance(seed, torch.Tensor) else None
    seed = 0 if seed_dev is not None else int(seed) & 0xFFFFFFFFFFFFFFFF
    if skip_self_loops or seed_dev is not None:
        L.check(lib.tfgx_asapstatic_attend_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), N, E, L.ptr(x), ldx, F, L.ptr(sq), L.ptr(sh),
                                               L.ptr(bias), float(drop_rate), seed, L.ptr(seed_dev), int(bool(skip_self_loops)),
                                               L.ptr(c), max(F, 1), L.ptr(p), L.ptr(p_self), L.ptr(pd), L.ptr(pds),
                                               L.ptr(bad_flag), L.stream_ptr()), "tfgx_asapstatic_attend_f32")
        return c, p, p_self, pd, pds
    L.check(lib.tfgx_asap_attend_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), N, E, L.ptr(x), ldx, F, L.ptr(sq), L.ptr(sh),
                                     L.ptr(bias), float(drop_rate), seed, L.ptr(c), max(F, 1),
                                     L.ptr(p), L.ptr(p_self), L.ptr(pd), L.ptr(pds), L.ptr(bad_flag), L.stream_ptr()),
            "tfgx_asap_attend_f32")
    return c, p, p_self, pd, pds


class _AsapAttend(torch.autograd.Function):
    """ASAP's 1-hop attention (include/tfgx_asap.h): c_i = sum_e k_e p_e x[col_e] over row i and its implicit self edge, with
    p = softmax_i(leaky_relu(sq_i + sh[col_e] + bias)).  Returns (c, k p [E], k p of the self edges [N]); only c carries a
    gradient (the weights feed the detached assignment).  Backward: d/dx on the transposed plan with k p as weights,
    dp_e = <g_i, x[col_e]> on the SDDMM kernel (both existing), then ONE launch for the softmax / leaky-relu backward."""

    @staticmethod
    def forward(ctx, plan, x, sq, sh, bias, drop_rate, seed, skip_self_loops=False):
        xd = x.detach()
        sqd, shd, bd = sq.detach().contiguous(), sh.detach().contiguous(), bias.detach().contiguous()
        c, p, p_self, pd, pds = asap_attend_forward(plan, xd, sqd, shd, bd, drop_rate, seed, skip_self_loops=skip_self_loops)
        ctx.plan, ctx.skip = plan, bool(skip_self_loops)
        ctx.save_for_backward(xd, sqd, shd, bd, p, p_self, pd, pds)
        pw, pws = (p, p_self) if pd is None else (pd, pds)
        ctx.mark_non_differentiable(pw, pws)
        return c, pw, pws

    @staticmethod
    def backward(ctx, g, _gp, _gps):
        lib = L.require_gpu()
        plan = ctx.plan
        x, sq, sh, bias, p, p_self, pd, pds = ctx.saved_tensors
        pw, pws = (p, p_self) if pd is None else (pd, pds)
        need_x = ctx.needs_input_grad[1]
        need_s = any(ctx.needs_input_grad[2:5])
        g = g.to(torch.float32).contiguous()
        gx, dp, dps = _aggregate_backward(plan, False, x, pw, pws, g, need_x, need_s, need_s)
        if not need_s:
            return None, gx, None, None, None, None, None, None
        N, E = plan.n_dst, plan.num_edges
        ds = torch.empty(E, dtype=torch.float32, device=g.device)
        ds_self = torch.empty(N, dtype=torch.float32, device=g.device)
        dsq = torch.empty(N, dtype=torch.float32, device=g.device)
        if ctx.skip:      # the fixed-shape route: the centred form, exact for a row of one term (include/tfgx_asap_static.h)
            L.check(lib.tfgx_asapstatic_attend_backward_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), N, E, L.ptr(sq), L.ptr(sh),
                                                            L.ptr(bias), L.ptr(p), L.ptr(p_self), L.ptr(pd), L.ptr(pds),
                                                            L.ptr(dp.contiguous()), L.ptr(dps.contiguous()), 1, L.ptr(ds),
                                                            L.ptr(ds_self), L.ptr(dsq), L.stream_ptr()),
                    "tfgx_asapstatic_attend_backward_f32")
        else:
            L.check(lib.tfgx_asap_attend_backward_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), N, E, L.ptr(sq), L.ptr(sh), L.ptr(bias),
                                                      L.ptr(p), L.ptr(p_self), L.ptr(pd), L.ptr(pds), L.ptr(dp.contiguous()),
                                                      L.ptr(dps.contiguous()), L.ptr(ds), L.ptr(ds_self), L.ptr(dsq),
                                                      L.stream_ptr()), "tfgx_asap_attend_backward_f32")
        # d sh_j = sum of ds over the edges that point AT j, plus j's self edge: a segment sum on the transposed plan
        pt, t2d = _transposed(plan)
        ones = torch.ones((N, 1), dtype=torch.float32, device=g.device)
        dsh = segment_reduce(pt, ones, L.SUM, w_csr=_permute(ds, t2d) if E else ds, self_coef=ds_self)[:, 0]
        return None, gx, dsq, dsh.contiguous(), dsq.sum().reshape(1), None, None, None


def asap_attend_composed(plan, x, sq, sh, bias, drop_rate=0.0, seed=0):
    """The same attention from operators that were here before the fused launch: two scalar gathers, leaky_relu, the
    segment softmax kernel over the row ids (explicit self edges appended), dropout by dropout_keep_scale and the weighted
    aggregation.  Used past TFGX_ASAP_MAX_FEATURES and as the comparator of tests / tools/bench_asap.py; makes [E]-sized
    intermediates only ([E, 2A] is avoided by the split of the score kernel, as in the fused route)."""
    from .nn.kernel.segment import segment_softmax as _segment_softmax
    N, E = plan.n_dst, plan.num_edges
    rows = plan_rows(plan)
    ar = torch.arange(N, dtype=torch.int64, device=x.device)
    z = torch.cat([sq[rows] + sh[plan.col.long()], sq + sh]) + bias
    s = torch.nn.functional.leaky_relu(z, 0.2)
    prob = _segment_softmax(s, torch.cat([rows, ar]).to(torch.int32), N)
    if drop_rate > 0.0:
        prob = prob * dropout_keep_scale(seed, torch.arange(E + N, dtype=torch.int64, device=x.device), drop_rate)
    pw, pws = prob[:E], prob[E:]
    c = aggregate(plan, x, L.SUM, w_csr=pw.contiguous(), self_coef=pws.contiguous())
    return c, pw.detach(), pws.detach()


ASAP_FUSED = True      # developer A/B switch: False sends every width down the composed route


def asap_attend(plan, x, sq, sh, bias, drop_rate=0.0, seed=0, skip_self_loops=False):
    """(c [N, F], k p [E] in the plan's CSR order, k p of the self edges [N]) — the fused launch up to
    TFGX_ASAP_MAX_FEATURES columns, the composed route past it.  sq, sh: [N]; bias: [1].  skip_self_loops (nn.asap_static): an
    edge row == col is absent; seed may then be a device tensor (nn.conv.gat.new_drop_seed inside a capture).  That form has
    the fused launch only."""
    static = skip_self_loops or isinstance(seed, torch.Tensor)
    if static and int(x.shape[1]) > L.ASAP_MAX_FEATURES:
        raise ValueError("asap_attend: x has {} columns, the fused attention takes {} (TFGX_ASAP_MAX_FEATURES) and the "
                         "fixed-shape route has no other".format(int(x.shape[1]), L.ASAP_MAX_FEATURES))
    if static or (ASAP_FUSED and int(x.shape[1]) <= L.ASAP_MAX_FEATURES):
        seed = seed if isinstance(seed, torch.Tensor) else int(seed)
        if needs_grad(x, sq, sh, bias):
            return _AsapAttend.apply(plan, x, sq, sh, bias, float(drop_rate), seed, bool(skip_self_loops))
        c, p, p_self, pd, pds = asap_attend_forward(plan, x.detach(), sq.detach().contiguous(), sh.detach().contiguous(),
                                                    bias.detach().contiguous(), drop_rate, seed, skip_self_loops=skip_self_loops)
        return (c, p, p_self) if pd is None else (c, pd, pds)
    return asap_attend_composed(plan, x, sq, sh, bias, drop_rate, seed)


def segment_gram_forward(graph_plan, S, Y, bad_flag=None):
    """One tfgx_segment_gram_f32 call on a graph plan (rows = graphs, col = node ids): out [G * K, W] with
    out[g K + k, w] = sum over the nodes n of graph g, in the plan's order, of S[n, k] Y[n, w]."""
    lib = L.require_gpu()
    S, lds = L.row_major_2d(S)
    Y, ldy = L.row_major_2d(Y)
    G, N, K, W = graph_plan.n_dst, int(S.shape[0]), int(S.shape[1]), int(Y.shape[1])
    if int(Y.shape[0]) != N or graph_plan.num_edges != N:
        raise ValueError("segment_gram: S has {} rows, Y {} and the graph plan names {} nodes".format(
            N, int(Y.shape[0]), graph_plan.num_edges))
    if not 1 <= K <= L.SEGGRAM_MAX_K:
        raise ValueError("segment_gram: {} clusters per graph, TFGX_SEGGRAM_MAX_K = {} is the limit".format(K, L.SEGGRAM_MAX_K))
    out = torch.empty((G * K, W), dtype=torch.float32, device=S.device)
    ws_bytes = lib.tfgx_segment_gram_workspace_bytes(N, G, K, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=S.device) if ws_bytes else None
    L.check(lib.tfgx_segment_gram_f32(L.ptr(graph_plan.row_ptr), L.ptr(graph_plan.col), G, N, L.ptr(S), lds, K, L.ptr(Y), ldy, W,
                                      L.ptr(out), max(W, 1), L.ptr(bad_flag), L.ptr(ws), ws_bytes, L.stream_ptr()),
            "tfgx_segment_gram_f32")
    return out


def segment_gram_backward(node_graph_index, G, S, Y, g, need_s=True, need_y=True, bad_flag=None):
    """One tfgx_segment_gram_backward_f32 call: (dS [N, K] or None, dY [N, W] or None) for the gradient g [G * K, W]."""
    lib = L.require_gpu()
    S, lds = L.row_major_2d(S)
    Y, ldy = L.row_major_2d(Y)
    g, ldg = L.row_major_2d(g)
    N, K, W = int(S.shape[0]), int(S.shape[1]), int(Y.shape[1])
    d_s = torch.empty((N, K), dtype=torch.float32, device=S.device) if need_s else None
    d_y = torch.empty((N, W), dtype=torch.float32, device=S.device) if need_y else None
    L.check(lib.tfgx_segment_gram_backward_f32(L.ptr(node_graph_index), N, G, L.ptr(S), lds, K, L.ptr(Y), ldy, W, L.ptr(g), ldg,
                                               L.ptr(d_s), K, L.ptr(d_y), max(W, 1), L.ptr(bad_flag), L.stream_ptr()),
            "tfgx_segment_gram_backward_f32")
    return d_s, d_y


class _SegmentGram(torch.autograd.Function):
    """out[g] = S_g^T Y_g per graph (include/tfgx_seggram.h): one launch pair forward, one launch backward, which skips
    whichever of dS / dY is not asked for.  When S and Y are the same tensor both gradients land on it (autograd adds them)."""

    @staticmethod
    def forward(ctx, graph_plan, node_graph_index, S, Y):
        sd, yd = S.detach(), Y.detach()
        ctx.graph_plan, ctx.ids = graph_plan, node_graph_index
        ctx.save_for_backward(sd, yd)
        return segment_gram_forward(graph_plan, sd, yd)

    @staticmethod
    def backward(ctx, g):
        sd, yd = ctx.saved_tensors
        need_s, need_y = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if not (need_s or need_y):
            return None, None, None, None
        d_s, d_y = segment_gram_backward(ctx.ids, ctx.graph_plan.n_dst, sd, yd, g.to(torch.float32), need_s, need_y)
        return None, None, d_s, d_y


def segment_gram(graph_plan, node_graph_index, S, Y):
    """[G * K, W] block rows S_g^T Y_g for S [N, K] (K <= TFGX_SEGGRAM_MAX_K), Y [N, W]; graph_plan = the CSR over graphs of
    node_graph_index (int32 [N] on the device, any order).  Differentiable in S and Y; bit-identical from run to run."""
    S, Y = L.as_f32(S), L.as_f32(Y)
    if needs_grad(S, Y):
        return _SegmentGram.apply(graph_plan, node_graph_index, S, Y)
    return segment_gram_forward(graph_plan, S, Y)


def gcn_norm_forward(plan, w, tw, col_degrees, norm, fill, diag, add_self_loop, renorm):
    """The two launches of the GCN normalisation (tfgx_segment_weight_sum_f32, tfgx_gcn_norm_edges_f32) on constants:
    (w_out[E] in CSR order, self_coef[n], row_deg, col_deg).  w: raw weights in CSR order or None (unweighted).
    col_degrees: the column degrees are wanted too (norm="both", sym=False), summed from tw = the same weights in the
    transposed plan's order (None with w); col_deg is None otherwise."""
    lib = L.require_gpu()
    n = plan.n_dst
    dev = plan.row_ptr.device
    row_deg = torch.empty(n, dtype=torch.float32, device=dev)
    L.check(lib.tfgx_segment_weight_sum_f32(L.ptr(plan.row_ptr), L.ptr(w), n, diag, L.ptr(row_deg), L.stream_ptr()),
            "tfgx_segment_weight_sum_f32")
    col_deg = None
    if col_degrees:
        tplan = plan.transposed()
        col_deg = torch.empty(tplan.n_dst, dtype=torch.float32, device=dev)
        L.check(lib.tfgx_segment_weight_sum_f32(L.ptr(tplan.row_ptr), L.ptr(tw), tplan.n_dst, diag, L.ptr(col_deg),
                                                L.stream_ptr()), "tfgx_segment_weight_sum_f32")
    w_out = torch.empty(plan.num_edges, dtype=torch.float32, device=dev)
    self_coef = torch.empty(n, dtype=torch.float32, device=dev)
    L.check(lib.tfgx_gcn_norm_edges_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), L.ptr(w), n, L.ptr(row_deg),
                                        L.ptr(col_deg), L.NORM_MODES[norm], fill, int(bool(add_self_loop)),
                                        int(bool(renorm)), L.ptr(w_out), L.ptr(self_coef), L.stream_ptr()),
            "tfgx_gcn_norm_edges_f32")
    return w_out, self_coef, row_deg, col_deg


def gcn_norm_backward(plan, w, row_deg, col_deg, norm, fill, add_self_loop, renorm, G, S, passes=L.NORMGRAD_ALL,
                      scratch=None):
    """d/dw (CSR order) of gcn_norm_forward given G = d/dw_out and S = d/dself_coef (None: no such gradient): the three
    launches of tfgx_gcn_norm_backward_f32 (include/tfgx_normgrad.h) — segmented sums over the plan and over the transposed
    plan in a fixed order, no atomics, no host synchronisation.  passes / scratch = (A, B, t, dw) of an earlier call: one
    launch alone on what that call left (tools/bench_gcn_norm_grad.py)."""
    lib = L.require_gpu()
    E = plan.num_edges
    dev = w.device
    if E == 0:
        return torch.empty(0, dtype=torch.float32, device=dev)
    mode = L.NORM_MODES[norm]
    n_rows, n_cols = plan.n_dst, plan.n_src
    pt, t2d = _transposed(plan) if mode != L.NORM_LEFT else (None, None)
    if scratch is None:
        new = lambda n: torch.empty(n, dtype=torch.float32, device=dev)      # noqa: E731
        scratch = (new(n_rows) if mode != L.NORM_RIGHT else None, new(n_cols) if pt is not None else None,
                   new(E) if pt is not None else None, new(E))
    A, B, t, dw = scratch
    L.check(lib.tfgx_gcn_norm_backward_f32(
        L.ptr(plan.row_ptr), L.ptr(plan.col), L.ptr(w), n_rows, n_cols, None if pt is None else L.ptr(pt.row_ptr), L.ptr(t2d),
        L.ptr(row_deg), L.ptr(col_deg), mode, fill, int(bool(add_self_loop)), int(bool(renorm)), L.ptr(G), L.ptr(S),
        L.ptr(A), L.ptr(B), L.ptr(t), L.ptr(dw), int(passes), L.stream_ptr()), "tfgx_gcn_norm_backward_f32")
    return dw


class _GcnNorm(torch.autograd.Function):
    """(w_out, self_coef) = the GCN normalisation of the raw weights w (CSR order): the forward is gcn_norm_forward on
    detached data — the bits of the untracked route — and the backward is tfgx_gcn_norm_backward_f32.  A factor the forward
    zeroed (the degree power was inf or NaN) has derivative zero, so the gradient of an isolated node's edges is finite."""

    @staticmethod
    def forward(ctx, plan, w, norm, sym, fill, diag, add_self_loop, renorm):
        wd = w.detach().contiguous()
        both_sides = norm == "both" and not sym
        tw = (_permute(wd, _transposed(plan)[1]) if plan.num_edges else wd) if both_sides else None
        w_out, self_coef, row_deg, col_deg = gcn_norm_forward(plan, wd, tw, both_sides, norm, fill, diag, add_self_loop, renorm)
        ctx.plan, ctx.cfg = plan, (norm, fill, add_self_loop, renorm)
        ctx.save_for_backward(wd, row_deg, col_deg)
        ctx.set_materialize_grads(False)
        return w_out, self_coef

    @staticmethod
    def backward(ctx, G, S):
        wd, row_deg, col_deg = ctx.saved_tensors
        norm, fill, add_self_loop, renorm = ctx.cfg
        if S is not None and not add_self_loop:
            S = None        # the coefficient is the constant 0 there
        if G is None and S is None:
            return (None,) * 8
        G = torch.zeros_like(wd) if G is None else L.as_f32(G).contiguous()
        S = None if S is None else L.as_f32(S).contiguous()
        dw = gcn_norm_backward(ctx.plan, wd, row_deg, col_deg, norm, fill, add_self_loop, renorm, G, S)
        return None, dw, None, None, None, None, None, None


def gcn_norm(plan, w, norm, sym, fill, diag, add_self_loop, renorm):
    """Differentiable GCN normalisation of tracked raw weights w (CSR order, e.g. from edge_attr_csr):
    (w_out, self_coef), both carrying the gradient to w."""
    return _GcnNorm.apply(plan, w, norm, bool(sym), float(fill), float(diag), bool(add_self_loop), bool(renorm))
