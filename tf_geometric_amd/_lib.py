# coding=utf-8
"""ctypes binding of the C ABI declared in include/tfgx.h (libtfgx.so, hand-written HIP for gfx950).

There is NO CPU fallback: if the library is missing, or there is no GPU, every operator raises.
PyTorch is used only as plumbing: device memory (torch.Tensor), streams, torch.distributed.
"""
import collections
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TFGX_LIB_PATH") or os.path.join(_HERE, "lib", "libtfgx.so")   # (override: developer A/B of kernel builds)

SUM, MEAN, MAX = 0, 1, 2
ACT_NONE, ACT_RELU = 0, 1
NORM_BOTH, NORM_LEFT, NORM_RIGHT = 0, 1, 2
NORM_MODES = {"both": NORM_BOTH, "left": NORM_LEFT, "right": NORM_RIGHT}


class TfgxError(RuntimeError):
    pass


ABI_VERSION = 114      # include/tfgx.h TFGX_ABI_VERSION: struct layouts / signatures bound below


class ReduceArgs(ctypes.Structure):
    """struct tfgx_reduce_args (include/tfgx.h)."""
    _fields_ = [
        ("row_begin", ctypes.c_void_p), ("row_end", ctypes.c_void_p), ("rp_stride", ctypes.c_int64),
        ("col", ctypes.c_void_p), ("w", ctypes.c_void_p), ("n_dst", ctypes.c_int64),
        ("x", ctypes.c_void_p), ("ldx", ctypes.c_int64), ("F", ctypes.c_int64),
        ("out", ctypes.c_void_p), ("ldo", ctypes.c_int64),
        ("op", ctypes.c_int32), ("act", ctypes.c_int32), ("accumulate", ctypes.c_int32), ("hub_threshold", ctypes.c_int32),
        ("self_coef", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("add_x", ctypes.c_void_p),
        ("ld_add", ctypes.c_int64), ("mean_count", ctypes.c_void_p),
        ("hub_rows", ctypes.c_void_p), ("hub_chunk_ptr", ctypes.c_void_p), ("hub_chunk_begin", ctypes.c_void_p),
        ("hub_chunk_end", ctypes.c_void_p), ("n_hub_rows", ctypes.c_int64), ("n_hub_chunks", ctypes.c_int64),
        ("hub_scratch", ctypes.c_void_p),
        ("x_tail", ctypes.c_void_p), ("ld_tail", ctypes.c_int64), ("f_main", ctypes.c_int64),
        ("edge_tail", ctypes.c_void_p), ("ld_edge_tail", ctypes.c_int64),
        ("row_order", ctypes.c_void_p),
        ("track", ctypes.c_void_p), ("ld_track", ctypes.c_int64), ("track_row_begin", ctypes.c_void_p),
        ("hub_order_slot", ctypes.c_void_p),
        ("wide_blocks", ctypes.c_int32), ("verify", ctypes.c_int32),
        ("verify_x", ctypes.c_void_p), ("ld_verify_x", ctypes.c_int64), ("n_verify", ctypes.c_int64),
        ("verify_word", ctypes.c_void_p),
    ]


class GatArgs(ctypes.Structure):
    """struct tfgx_gat_args (include/tfgx.h)."""
    _fields_ = [
        ("row_ptr", ctypes.c_void_p), ("col", ctypes.c_void_p), ("n_dst", ctypes.c_int64),
        ("q", ctypes.c_void_p), ("ldq", ctypes.c_int64),
        ("k", ctypes.c_void_p), ("ldk", ctypes.c_int64),
        ("v", ctypes.c_void_p), ("ldv", ctypes.c_int64),
        ("out", ctypes.c_void_p), ("ldo", ctypes.c_int64),
        ("H", ctypes.c_int32), ("d", ctypes.c_int32), ("dv", ctypes.c_int32), ("add_self_loop", ctypes.c_int32),
        ("scale", ctypes.c_float), ("act", ctypes.c_int32), ("bias", ctypes.c_void_p),
        ("row_begin", ctypes.c_void_p), ("row_end", ctypes.c_void_p), ("rp_stride", ctypes.c_int64),
        ("state_acc", ctypes.c_void_p), ("state_ml", ctypes.c_void_p),
        ("hub_threshold", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("hub_rows", ctypes.c_void_p), ("hub_chunk_ptr", ctypes.c_void_p), ("hub_chunk_begin", ctypes.c_void_p),
        ("hub_chunk_end", ctypes.c_void_p), ("hub_chunk_row", ctypes.c_void_p),
        ("n_hub_rows", ctypes.c_int64), ("n_hub_chunks", ctypes.c_int64),
        ("hub_scratch_acc", ctypes.c_void_p), ("hub_scratch_ml", ctypes.c_void_p),
        ("stats_ml", ctypes.c_void_p),
        ("drop_rate", ctypes.c_float), ("reserved2", ctypes.c_int32), ("drop_seed", ctypes.c_uint64),
        ("drop_self_base", ctypes.c_int64),
        ("row_order", ctypes.c_void_p),
        ("drop_seed_dev", ctypes.c_void_p),
        ("state_in_acc", ctypes.c_void_p), ("state_in_ml", ctypes.c_void_p),
        ("qgrad_t", ctypes.c_void_p), ("qgrad_s", ctypes.c_void_p), ("state_t", ctypes.c_void_p), ("state_s", ctypes.c_void_p),
        ("state_in_t", ctypes.c_void_p), ("state_in_s", ctypes.c_void_p),
    ]


class HubLists(ctypes.Structure):
    """struct tfgx_hub_lists (include/tfgx.h)."""
    _fields_ = [("threshold", ctypes.c_int32), ("reserved", ctypes.c_int32), ("n_rows", ctypes.c_int64),
                ("n_chunks", ctypes.c_int64), ("rows", ctypes.c_void_p), ("chunk_ptr", ctypes.c_void_p),
                ("chunk_begin", ctypes.c_void_p), ("chunk_end", ctypes.c_void_p), ("chunk_row", ctypes.c_void_p)]


def edge_softmax(plan, score, H, out):
    """tfgx_edge_softmax_hub_f32 on `plan` (hub rows chunk-wise when the plan has any)."""
    lib = require_gpu()
    hub, nc = hub_lists(plan)
    hp = 1
    while hp < H:
        hp <<= 1
    scratch = torch.empty(max(nc * 2 * hp, 1), dtype=torch.float32, device=out.device) if hub is not None else None
    check(lib.tfgx_edge_softmax_hub_f32(ptr(plan.row_ptr), ptr(plan.perm), ptr(score), H, plan.n_dst, ptr(out),
                                        None if hub is None else ctypes.byref(hub), ptr(scratch), stream_ptr()),
          "tfgx_edge_softmax_hub_f32")
    return out


def hub_lists(plan):
    """(HubLists struct, n_chunks) of a plan's long rows, or (None, 0) when the plan has none (plan.hub_info())."""
    info = plan.hub_info()
    if info is None:
        return None, 0
    hub_rows, chunk_ptr, chunk_begin, chunk_end, chunk_row = info
    h = HubLists()
    h.threshold, h.n_rows, h.n_chunks = int(plan.hub_threshold), int(hub_rows.shape[0]), int(chunk_begin.shape[0])
    h.rows, h.chunk_ptr = hub_rows.data_ptr(), chunk_ptr.data_ptr()
    h.chunk_begin, h.chunk_end, h.chunk_row = chunk_begin.data_ptr(), chunk_end.data_ptr(), chunk_row.data_ptr()
    return h, int(chunk_begin.shape[0])


class GatBackwardArgs(ctypes.Structure):
    """struct tfgx_gat_backward_args (include/tfgx.h)."""
    _fields_ = [
        ("row_ptr", ctypes.c_void_p), ("col", ctypes.c_void_p), ("n_dst", ctypes.c_int64),
        ("row_ptr_t", ctypes.c_void_p), ("dst_t", ctypes.c_void_p), ("n_src", ctypes.c_int64),
        ("q", ctypes.c_void_p), ("ldq", ctypes.c_int64),
        ("k", ctypes.c_void_p), ("ldk", ctypes.c_int64),
        ("v", ctypes.c_void_p), ("ldv", ctypes.c_int64),
        ("grad_out", ctypes.c_void_p), ("ld_grad_out", ctypes.c_int64),
        ("stats_ml", ctypes.c_void_p), ("dsum", ctypes.c_void_p),
        ("H", ctypes.c_int32), ("d", ctypes.c_int32), ("dv", ctypes.c_int32), ("add_self_loop", ctypes.c_int32),
        ("scale", ctypes.c_float), ("reserved", ctypes.c_int32),
        ("grad_q", ctypes.c_void_p), ("ld_grad_q", ctypes.c_int64),
        ("grad_k", ctypes.c_void_p), ("ld_grad_k", ctypes.c_int64),
        ("grad_v", ctypes.c_void_p), ("ld_grad_v", ctypes.c_int64),
        ("drop_rate", ctypes.c_float), ("reserved2", ctypes.c_int32), ("drop_seed", ctypes.c_uint64),
        ("drop_self_base", ctypes.c_int64), ("edge_pos_t", ctypes.c_void_p),
        ("ld_stats_ml", ctypes.c_int64), ("ld_dsum", ctypes.c_int64),
        ("row_order", ctypes.c_void_p), ("row_order_t", ctypes.c_void_p),
        ("drop_seed_dev", ctypes.c_void_p),
        ("span_begin", ctypes.c_void_p), ("span_end", ctypes.c_void_p), ("span_stride", ctypes.c_int64),
        ("accumulate", ctypes.c_int32), ("reserved3", ctypes.c_int32),
        ("head_pack", ctypes.c_void_p), ("ld_head_pack", ctypes.c_int64),
    ]


# name -> (restype, argtypes); every table is checked against its header, type by type, by tests/test_abi_registry.py
_I64, _I32, _F32, _P, _SZ = ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
SIGNATURES = {
    "tfgx_version": (ctypes.c_int, []),
    "tfgx_column_sum_workspace_bytes": (_SZ, [_I64, _I64]),
    "tfgx_column_sum_f32": (ctypes.c_int, [_P, _I64, _I64, _I64, _P, _P, _SZ, _P]),
    "tfgx_last_error": (ctypes.c_char_p, []),
    "tfgx_csr_plan_workspace_bytes": (_SZ, [_I64, _I64]),
    "tfgx_build_csr_by_dst": (ctypes.c_int, [_P, _P, _I64, _I64, _I64, _P, _P, _P, _P, _SZ, _P]),
    "tfgx_merge_edges_workspace_bytes": (_SZ, [_I64, _I64]),
    "tfgx_merge_duplicated_edges": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _P, _P, _P, _P, _SZ, _P]),
    "tfgx_segment_topk_workspace_bytes": (_SZ, [_I64, _I64]),
    "tfgx_segment_topk": (ctypes.c_int, [_P, _P, _I64, _I64, _I32, _F32, _P, _P, _P, _SZ, _P]),
    "tfgx_segment_max_with_count_f32": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P]),
    "tfgx_segment_max_with_arg_f32": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P, _I64, _P]),
    "tfgx_segment_max_backward_mask_workspace_bytes": (_SZ, [_I64, _I64, _I64]),
    "tfgx_pool_mlp_max_wgrad_applies": (ctypes.c_int, [_I64, _I64]),
    "tfgx_pool_mlp_max_wgrad_plan_bytes": (_SZ, [_I64, _I64, _I64, _I64]),
    "tfgx_pool_mlp_max_wgrad_plan": (ctypes.c_int, [_P, _I64, _I64, _I64, _I64, _P, _SZ, _P]),
    "tfgx_pool_mlp_max_wgrad_workspace_bytes": (_SZ, [_I64, _I64, _I64]),
    "tfgx_pool_mlp_max_wgrad_f32": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _I64,
                                                   _P, _P, _I64, _P, _P, _SZ, _P]),
    "tfgx_segment_max_backward_mask_f32": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P,
                                                          _I64, _P, _I64, _P, _P, _P, _P, _I64, _P, _I64, _P, _SZ, _P]),
    "tfgx_segment_max_backward_mask_phases_f32": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P,
                                                                 _I64, _P, _I64, _P, _P, _P, _P, _I64, _P, _I64, _P, _SZ,
                                                                 ctypes.c_int32, _P]),
    "tfgx_segment_max_backward_push_f32": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P,
                                                          _I64, _P, _I64, _P, _I64, _P]),
    "tfgx_segment_max_backward_w_f32": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P, _P]),
    "tfgx_gemm_workspace_bytes": (_SZ, [_I64, _I64, _I64]),
    "tfgx_gemm_tn_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I32]),
    "tfgx_gemm_tn_f32": (ctypes.c_int, [_P, _I64, _P, _I64, _I64, _I64, _I64, _P, _I64, _P, _P, _SZ, _P]),
    "tfgx_gemm_tn_gated_f32": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _I64, _I64, _I64, _P, _I64, _P, _P, _SZ, _P]),
    "tfgx_transpose_f32": (ctypes.c_int, [_P, _I64, _I64, _I64, _P, _I64, _P]),
    "tfgx_gemm_bias_act_cols_ws_f32": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I32, _I64, _P, _I64, _I64, _I64, _I64, _P, _SZ, _P]),
    "tfgx_gemm_describe": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I32, _I64, _P, _I64, _I64, _I64, _I64, _P, _SZ, ctypes.c_char_p,
                                          ctypes.c_size_t]),
    "tfgx_dropout_keep": (ctypes.c_int32, [ctypes.c_uint64, ctypes.c_uint32, _F32]),
    "tfgx_permute_rows_f32": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _P]),
    "tfgx_gat_pack_dst_f32": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _I32, _I32, _I32, _P, _I64, _P, _P]),
    "tfgx_gat_query_grad_d1_f32": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _P, _I64, _I32, _I32, ctypes.c_float, _P, _I64, _P]),
    "tfgx_gat_pack_dst_heads_f32": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _I32, _I32, _I32, _P, _I64, _P, _P]),
    "tfgx_relu_backward_f32": (ctypes.c_int, [_P, _I64, _P, _I64, _I64, _I64, _P, _I64, _P]),
    "tfgx_scatter_add_rows_f32": (ctypes.c_int, [_P, _I64, _P, _I64, _I64, _P, _I64, _P]),
    "tfgx_segment_reduce_f32": (ctypes.c_int, [ctypes.POINTER(ReduceArgs), _P]),
    "tfgx_segment_reduce_describe": (ctypes.c_int, [ctypes.POINTER(ReduceArgs), ctypes.c_char_p, ctypes.c_size_t]),
    "tfgx_segment_weight_sum_f32": (ctypes.c_int, [_P, _P, _I64, _F32, _P, _P]),
    "tfgx_gcn_norm_edges_f32": (ctypes.c_int, [_P, _P, _P, _I64, _P, _P, _I32, _F32, _I32, _I32, _P, _P, _P]),
    "tfgx_edge_softmax_f32": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _P, _P]),
    "tfgx_gat_fused_f32": (ctypes.c_int, [ctypes.POINTER(GatArgs), _P]),
    "tfgx_gat_merge_passes_f32": (ctypes.c_int, [ctypes.POINTER(GatArgs), _P, _P, _I32, _P]),
    "tfgx_gat_merge_parts_f32": (ctypes.c_int, [ctypes.POINTER(GatArgs), _P, _P, _P, _P, _P]),
    "tfgx_sddmm_f32": (ctypes.c_int, [_P, _P, _I64, _P, _I64, _P, _I64, _I64, _P, _P]),
    "tfgx_segment_max_count_f32": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P]),
    "tfgx_segment_max_backward_f32": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P, _I64,
                                                     _P, _I64, _I64, _P, _P]),
    "tfgx_gat_backward_dst_f32": (ctypes.c_int, [ctypes.POINTER(GatBackwardArgs), _P]),
    "tfgx_gat_backward_src_f32": (ctypes.c_int, [ctypes.POINTER(GatBackwardArgs), _P]),
    "tfgx_edge_softmax_hub_f32": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _P, ctypes.POINTER(HubLists), _P, _P]),
    "tfgx_sddmm_hub_f32": (ctypes.c_int, [_P, _P, _I64, _P, _I64, _P, _I64, _I64, _P, ctypes.POINTER(HubLists), _P]),
    "tfgx_gat_backward_dst_hub_f32": (ctypes.c_int, [ctypes.POINTER(GatBackwardArgs), ctypes.POINTER(HubLists), _P, _P]),
    "tfgx_gat_backward_src_hub_f32": (ctypes.c_int, [ctypes.POINTER(GatBackwardArgs), ctypes.POINTER(HubLists), _P, _P]),
    "tfgx_segment_max_count_hub_f32": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _I64, _P, _I64, _P, _I64,
                                                      ctypes.POINTER(HubLists), _P, _P]),
    "tfgx_segment_max_backward_hub_f32": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P, _I64,
                                                         _P, _I64, _I64, _P, ctypes.POINTER(HubLists), _P, _P]),
    "tfgx_head_mean_f32": (ctypes.c_int, [_P, _I64, _I64, _I32, _I32, _P, _I32, _P, _I64, _P]),
    "tfgx_gemm_bias_act_f32": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I32, _P, _I64, _I64, _I64, _I64, _P]),
    "tfgx_gemm_bias_act_cols_f32": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I32, _I64, _P, _I64, _I64, _I64, _I64, _P]),
    "tfgx_l2_normalize_rows_f32": (ctypes.c_int, [_P, _I64, _I64, _I64, _P]),
    "tfgx_sample_neighbors": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I32, _I32, ctypes.c_uint64, _P, _P, _P]),
    "tfgx_induced_subgraph_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I32]),
    "tfgx_induced_subgraph_count": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _I64, _P, ctypes.POINTER(ctypes.c_int64), _P,
                                                   _SZ, _P]),
    "tfgx_induced_subgraph_emit": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                  _P, _SZ, _P]),
    "tfgx_gather_i32": (ctypes.c_int, [_P, _P, _I64, _P, _P]),
    "tfgx_gather_scale_rows_f32": (ctypes.c_int, [_P, _I64, _P, _P, _I64, _I64, _P, _I64, _P]),
    "tfgx_gather_scale_rows_backward_f32": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _P]),
    "tfgx_split_rows_f32": (ctypes.c_int, [_P, _I64, _I64, _I64, _I64, _P, _I64, _P, _I64, _P]),
    "tfgx_split_rows_verify_f32": (ctypes.c_int, [_P, _I64, _I64, _I64, _I64, _P, _I64, _P, _I64, _I64, ctypes.c_uint64, _P, _P]),
    "tfgx_gather_rows_f32": (ctypes.c_int, [_P, _I64, _P, _I64, _I64, _P, _I64, _P]),
    "tfgx_halo_workspace_bytes": (_SZ, [_I64]),
    "tfgx_halo_mark": (ctypes.c_int, [_P, _I64, _I32, _I32, _I64, _P, _P]),
    "tfgx_halo_compact": (ctypes.c_int, [_P, _I64, _P, _P, _P, _P, _SZ, _P]),
    "tfgx_halo_remap_cols": (ctypes.c_int, [_P, _I64, _I32, _I32, _P, _I32, _P, _P]),
    "tfgx_split_by_source_class": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _P, _I32, _P, _P, _P, _P]),
    "tfgx_aggregate_gemm_fits": (ctypes.c_int, [_I64, _I64]),
    "tfgx_aggregate_gemm_f32": (ctypes.c_int, [ctypes.POINTER(ReduceArgs), _P, _I64, _P, _I32, _P, _I64, _I64, _P]),
    "tfgx_hub_policy": (ctypes.c_int, [_I64, _I64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "tfgx_gat_source_block_count": (ctypes.c_int32, [_I64, _I64, _I64, _I64, _I64, _I64, _I64]),
    "tfgx_plan_row_order_workspace_bytes": (_SZ, [_I64]),
    "tfgx_plan_row_order": (ctypes.c_int, [_P, _I64, _I64, _P, ctypes.POINTER(ctypes.c_int32), _P, _SZ, _P]),
    "tfgx_plan_hub_lists_workspace_bytes": (_SZ, [_I64]),
    "tfgx_plan_hub_lists_count": (ctypes.c_int, [_P, _P, _I64, _I64, _I32, _I32, ctypes.POINTER(ctypes.c_int64),
                                                 ctypes.POINTER(ctypes.c_int64), _P, _SZ, _P]),
    "tfgx_plan_hub_lists_emit": (ctypes.c_int, [_P, _P, _I64, _I64, _I32, _I32, _I64, _I64, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "tfgx_plan_hub_order_slot": (ctypes.c_int, [_P, _I64, _P, _P, _P]),
    "tfgx_plan_source_blocks": (ctypes.c_int, [_P, _P, _I64, _I64, _I64, _I32, _P, _P, _P]),
}

# include/tfgx_h16.h (16-bit feature tables)
H16_ABI_VERSION = 1
DT_F32, DT_BF16, DT_F16 = 0, 1, 2
H16_DTYPES = {torch.bfloat16: DT_BF16, torch.float16: DT_F16}
H16_SIGNATURES = {
    "tfgx_h16_version": (ctypes.c_int, []),
    "tfgx_segment_reduce_h16": (ctypes.c_int, [ctypes.POINTER(ReduceArgs), _I32, _I32, _P]),
    "tfgx_segment_reduce_h16_describe": (ctypes.c_int, [ctypes.POINTER(ReduceArgs), _I32, _I32, ctypes.c_char_p, ctypes.c_size_t]),
    "tfgx_rows_f32_to_h16": (ctypes.c_int, [_P, _I64, _I64, _I64, _P, _I64, _I32, _P]),
    "tfgx_rows_h16_to_f32": (ctypes.c_int, [_P, _I64, _I32, _I64, _I64, _P, _I64, _P]),
    "tfgx_h16_friendly_ld": (_I64, [_I64]),
}

# include/tfgx_fused_h16.h (the fused aggregate -> project launch over a 16-bit table)
FUSED_H16_ABI_VERSION = 1
FUSED_H16_SIGNATURES = {
    "tfgx_fused_h16_version": (ctypes.c_int, []),
    "tfgx_aggregate_gemm_h16": (ctypes.c_int, [ctypes.POINTER(ReduceArgs), _I32, _P, _I64, _P, _I32, _P, _I64, _I64, _P]),
    "tfgx_aggregate_gemm_h16_describe": (ctypes.c_int, [ctypes.POINTER(ReduceArgs), _I32, _I64, ctypes.c_char_p, ctypes.c_size_t]),
}

# include/tfgx_gemm_h16.h (the dense GEMM and its weight gradient reading a 16-bit table)
GEMM_H16_ABI_VERSION = 1
GEMM_H16_SIGNATURES = {
    "tfgx_gemm_h16_version": (ctypes.c_int, []),
    "tfgx_gemm_bias_act_cols_ws_h16": (ctypes.c_int, [_P, _I32, _I64, _P, _I64, _P, _I32, _I64, _P, _I64, _I64, _I64, _I64, _P, _SZ,
                                                      _P]),
    "tfgx_gemm_h16_describe": (ctypes.c_int, [_P, _I32, _I64, _P, _I64, _P, _I32, _I64, _P, _I64, _I64, _I64, _I64, _P, _SZ,
                                              ctypes.c_char_p, ctypes.c_size_t]),
    "tfgx_gemm_tn_gated_h16": (ctypes.c_int, [_P, _I32, _I64, _P, _I64, _P, _I64, _I64, _I64, _I64, _P, _I64, _P, _P, _SZ, _P]),
}



class DropEdgePlan(ctypes.Structure):
    """struct tfgx_drop_edge_plan (include/tfgx_dropedge.h)."""
    _fields_ = [("parent_row_ptr", ctypes.c_void_p), ("parent_col", ctypes.c_void_p), ("parent_perm", ctypes.c_void_p),
                ("out_row_ptr", ctypes.c_void_p), ("out_col", ctypes.c_void_p), ("out_perm", ctypes.c_void_p)]


# include/tfgx_dropedge.h (DropEdge: edge dropout with sort-free plans)
DROPEDGE_ABI_VERSION = 1
DROPEDGE_SIGNATURES = {
    "tfgx_dropedge_version": (ctypes.c_int, []),
    "tfgx_drop_edge_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I32, _I32]),
    "tfgx_drop_edge_count": (ctypes.c_int, [_P, _P, _I64, _I64, _I64, _F32, ctypes.c_uint64, _I32, ctypes.POINTER(ctypes.c_int64),
                                            _P, _SZ, _P]),
    "tfgx_drop_edge_emit": (ctypes.c_int, [_P, _P, _I64, _I64, _I64, _F32, ctypes.c_uint64, _I32, _I64, _P, _P, _P,
                                           ctypes.POINTER(DropEdgePlan), ctypes.POINTER(DropEdgePlan), _P, _SZ, _P]),
}

# include/tfgx_linkpred.h (link prediction: the per-edge decoder and the negative samplers)
LINKPRED_ABI_VERSION = 1
NEGATIVE_BAD_START = -(1 << 31)     # TFGX_NEGATIVE_BAD_START as the int32 the device word is read as
_U64, _U32 = ctypes.c_uint64, ctypes.c_uint32
LINKPRED_SIGNATURES = {
    "tfgx_linkpred_version": (ctypes.c_int, []),
    "tfgx_edge_dot_f32": (ctypes.c_int, [_P, _P, _I64, _P, _I64, _I64, _P, _I64, _I64, _I64, _P, _P, _P]),
    "tfgx_negative_draw": (None, [_U64, _U64, _U32, _I64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "tfgx_negative_sample_pairs": (ctypes.c_int, [_I64, _I64, _P, _P, _I32, _U64, _U64, _I32, _P, _P, _P, _P]),
    "tfgx_negative_sample_from": (ctypes.c_int, [_P, _I64, _I64, _P, _P, _U64, _U64, _I32, _P, _P, _P]),
}

# include/tfgx_lstm.h (the LSTM GraphSAGE aggregator: fused gather -> recurrence and its backward through time)
LSTM_ABI_VERSION = 1
LSTM_MAX_UNITS = 256
LSTM_SIGNATURES = {
    "tfgx_lstm_version": (ctypes.c_int, []),
    "tfgx_lstm_recurrent_kernel_resident": (ctypes.c_int, [_I64, _I32]),
    "tfgx_lstm_aggregate_saved_bytes": (_SZ, [_I64, _I64, _I64]),
    "tfgx_lstm_aggregate_tiles": (_I64, [_I64]),
    "tfgx_lstm_aggregate_f32": (ctypes.c_int, [_P, _P, _I64, _I64, _I64, _P, _I64, _P, _P, _I64, _P, _I64, _P, _SZ, _P, _P]),
    "tfgx_lstm_aggregate_backward_f32": (ctypes.c_int, [_P, _I64, _I64, _I64, _P, _P, _I64, _P, _SZ, _P, _P, _P, _P]),
}

# include/tfgx_set2set.h (Set2Set: the per-graph attention readout and the stateful sequence LSTM, each with its backward)
SET2SET_ABI_VERSION = 1
SET2SET_CHUNK_ROWS = 512
SET2SET_MAX_FEATURES = 1024
SET2SET_SIGNATURES = {
    "tfgx_set2set_version": (ctypes.c_int, []),
    "tfgx_set2set_attend_workspace_bytes": (_SZ, [_I64, _I64, _I64]),
    "tfgx_set2set_attend_f32": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P, _P, _SZ, _P, _P]),
    "tfgx_set2set_attend_backward_f32": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P, _P, _I64,
                                                        _P, _I64, _P, _I64, _P, _SZ, _P]),
    "tfgx_lstm_sequence_kernel_resident": (ctypes.c_int, [_I64]),
    "tfgx_lstm_sequence_saved_bytes": (_SZ, [_I64, _I64, _I64]),
    "tfgx_lstm_sequence_f32": (ctypes.c_int, [_P, _I64, _I64, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "tfgx_lstm_sequence_backward_f32": (ctypes.c_int, [_I64, _I64, _I64, _P, _P, _P, _P, _P, _P, _SZ, _P, _P, _P, _P, _P]),
}

# include/tfgx_asap.h (ASAP pooling: the fused 1-hop attention with its backward, and the sparse S^T A S of cluster_pool)
ASAP_ABI_VERSION = 1
ASAP_MAX_FEATURES = 256
_PI64 = ctypes.POINTER(ctypes.c_int64)
ASAP_SIGNATURES = {
    "tfgx_asap_version": (ctypes.c_int, []),
    "tfgx_asap_attend_f32": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _I64, _I64, _P, _P, _P, _F32, _U64, _P, _I64, _P, _P, _P, _P,
                                            _P, _P]),
    "tfgx_asap_attend_backward_f32": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "tfgx_spasp_count_workspace_bytes": (_SZ, [_I64, _I64]),
    "tfgx_spasp_workspace_bytes": (_SZ, [_I64, _I64]),
    "tfgx_spasp_count": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _P, _I64, _P, _P, _PI64, _P, _SZ, _P]),
    "tfgx_spasp_emit": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _P, _P, _P, _I64, _P, _P, _I64, _P, _SZ, _P]),
    "tfgx_spasp_reduce": (ctypes.c_int, [_I64, _I64, _I32, _P, _P, _P, _P, _P, _P, _SZ, _P]),
}

# include/tfgx_seggram.h (the segmented transposed product S_g^T Y_g of DiffPool / MinCutPool and its backward)
SEGGRAM_ABI_VERSION = 1
SEGGRAM_MAX_K = 64
SEGGRAM_BLOCK = 64
SEGGRAM_SIGNATURES = {
    "tfgx_seggram_version": (ctypes.c_int, []),
    "tfgx_seggram_block": (ctypes.c_int, []),
    "tfgx_segment_gram_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I64]),
    "tfgx_segment_gram_f32": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _P, _P, _SZ, _P]),
    "tfgx_segment_gram_backward_f32": (ctypes.c_int, [_P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P,
                                                      _I64, _P, _P]),
}

# include/tfgx_normgrad.h (the backward of the GCN normalisation: d/d raw edge weights)
NORMGRAD_ABI_VERSION = 1
NORMGRAD_ROW_PASS, NORMGRAD_COL_PASS, NORMGRAD_EDGE_PASS, NORMGRAD_ALL = 1, 2, 4, 7
NORMGRAD_SIGNATURES = {
    "tfgx_normgrad_version": (ctypes.c_int, []),
    "tfgx_gcn_norm_backward_f32": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _P, _P, _P, _P, _I32, _F32, _I32, _I32, _P, _P, _P, _P,
                                                  _P, _P, _I32, _P]),
}



class CollatePlan(ctypes.Structure):
    """struct tfgx_collate_plan (include/tfgx_collate.h)."""
    _fields_ = [("ds_row_ptr", ctypes.c_void_p), ("ds_col", ctypes.c_void_p), ("ds_perm", ctypes.c_void_p),
                ("out_row_ptr", ctypes.c_void_p), ("out_col", ctypes.c_void_p), ("out_perm", ctypes.c_void_p)]


class CollateArgs(ctypes.Structure):
    """struct tfgx_collate_args (include/tfgx_collate.h)."""
    _fields_ = [
        ("ds_x", ctypes.c_void_p), ("ds_ldx", ctypes.c_int64), ("F", ctypes.c_int64),
        ("ds_row", ctypes.c_void_p), ("ds_col", ctypes.c_void_p), ("ds_w", ctypes.c_void_p),
        ("ds_n", ctypes.c_int64), ("ds_e", ctypes.c_int64),
        ("table", ctypes.c_void_p), ("B", ctypes.c_int64), ("n_out", ctypes.c_int64), ("e_out", ctypes.c_int64),
        ("out_x", ctypes.c_void_p), ("out_ldx", ctypes.c_int64), ("out_node_graph_index", ctypes.c_void_p),
        ("out_row", ctypes.c_void_p), ("out_col", ctypes.c_void_p), ("out_edge_graph_index", ctypes.c_void_p),
        ("out_w", ctypes.c_void_p),
        ("plan", ctypes.POINTER(CollatePlan)), ("plan_t", ctypes.POINTER(CollatePlan)),
    ]


class CollateStaticArgs(ctypes.Structure):
    """struct tfgx_static_batch_args (include/tfgx_collate_static.h)."""
    _fields_ = [
        ("ds_x", ctypes.c_void_p), ("ds_ldx", ctypes.c_int64), ("F", ctypes.c_int64),
        ("ds_row", ctypes.c_void_p), ("ds_col", ctypes.c_void_p), ("ds_w", ctypes.c_void_p),
        ("ds_n", ctypes.c_int64), ("ds_e", ctypes.c_int64),
        ("table", ctypes.c_void_p), ("B", ctypes.c_int64),
        ("n_cap", ctypes.c_int64), ("e_cap", ctypes.c_int64), ("sinks", ctypes.c_int64), ("sink_degree", ctypes.c_int64),
        ("out_x", ctypes.c_void_p), ("out_ldx", ctypes.c_int64), ("out_node_graph_index", ctypes.c_void_p),
        ("out_row", ctypes.c_void_p), ("out_col", ctypes.c_void_p), ("out_edge_graph_index", ctypes.c_void_p),
        ("out_w", ctypes.c_void_p),
        ("plan", ctypes.POINTER(CollatePlan)), ("plan_t", ctypes.POINTER(CollatePlan)),
        ("graph_row_ptr", ctypes.c_void_p),
    ]


# include/tfgx_collate.h (minibatch assembly out of a packed device dataset, with sort-free plans)
COLLATE_ABI_VERSION = 1
COLLATE_TILE = 1024          # TFGX_COLLATE_TILE: output elements per workgroup
COLLATE_SIGNATURES = {
    "tfgx_collate_version": (ctypes.c_int, []),
    "tfgx_collate_tile": (ctypes.c_int, []),
    "tfgx_collate": (ctypes.c_int, [ctypes.POINTER(CollateArgs), _P]),
}

# include/tfgx_nbrblock.h (minibatch neighbour sampling: the row-list sampler and the order-stable relabel over a persistent
# table)
NBRBLOCK_ABI_VERSION = 1
NBRBLOCK_EMPTY = (1 << 31) - 1     # TFGX_NBRBLOCK_EMPTY: a table entry without a virtual id
NBRBLOCK_BAD_RANGE, NBRBLOCK_BAD_REPEAT = 1, 2
NBRBLOCK_SIGNATURES = {
    "tfgx_nbrblock_version": (ctypes.c_int, []),
    "tfgx_nbrblock_sample_rows": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _P, _I32, _U64, _P, _P, _P, _P]),
    "tfgx_nbrblock_stamp": (ctypes.c_int, [_P, _I64, _P, _I64, _I64, _P, _P]),
    "tfgx_nbrblock_relabel_workspace_bytes": (_SZ, [_I64]),
    "tfgx_nbrblock_relabel": (ctypes.c_int, [_P, _I64, _I64, _P, _I64, _P, _P, _P, _P, _SZ, _P]),
    "tfgx_nbrblock_reset": (ctypes.c_int, [_P, _I64, _P, _I64, _P]),
}

# include/tfgx_samplereduce.h (the fused input hop of minibatch GraphSAGE: draw a listed node's neighbours and reduce their
# feature rows in one launch)
SAMPLEREDUCE_ABI_VERSION = 1
SAMPLEREDUCE_MAX_DRAWS = 256       # TFGX_SAMPLEREDUCE_MAX_DRAWS: the largest k whose drawn list the kernel keeps in LDS
SAMPLEREDUCE_BAD_RANGE = NBRBLOCK_BAD_RANGE
SAMPLEREDUCE_SIGNATURES = {
    "tfgx_samplereduce_version": (ctypes.c_int, []),
    "tfgx_samplereduce_f32": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _I32, _I32, _U64, _P, _I64, _I64, _I32, _P, _I64, _P, _P,
                                             _P]),
}

# include/tfgx_nbrstatic.h (fixed-shape minibatch sampling: capacities the host knows, run-time sizes on the device, no reads)
NBRSTATIC_ABI_VERSION = 1
NBRSTATIC_DEAD = -1                # TFGX_NBRSTATIC_DEAD: a dead seed slot / virtual node
NBRSTATIC_BAD_RANGE, NBRSTATIC_BAD_REPEAT = NBRBLOCK_BAD_RANGE, NBRBLOCK_BAD_REPEAT
NBRSTATIC_SIGNATURES = {
    "tfgx_nbrstatic_version": (ctypes.c_int, []),
    "tfgx_nbrstatic_seeds": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _P, _P]),
    "tfgx_nbrstatic_hop_workspace_bytes": (_SZ, [_I64, _I32]),
    "tfgx_nbrstatic_hop": (ctypes.c_int, [_P, _P, _P, _I64, _P, _P, _I64, _I32, _I32, _P, _I32, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "tfgx_nbrstatic_transpose_workspace_bytes": (_SZ, [_I64, _I64]),
    "tfgx_nbrstatic_transpose": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _P, _P, _P, _SZ, _P]),
    "tfgx_nbrstatic_gather_rows_f32": (ctypes.c_int, [_P, _I64, _P, _I64, _I64, _P, _I64, _P]),
    "tfgx_nbrstatic_input_hop_f32": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _I32, _I32, _P, _I32, _P, _I64, _I64, _I32, _P, _I64,
                                                    _P, _P, _P]),
}

# include/tfgx_minibatch_h16.h (the minibatch route over a 16-bit feature table: the fused input hop in both forms, the gather)
MINIBATCH_H16_ABI_VERSION = 1
MINIBATCH_H16_SIGNATURES = {
    "tfgx_minibatch_h16_version": (ctypes.c_int, []),
    "tfgx_sample_reduce_h16": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _I32, _I32, _U64, _P, _I64, _I64, _I32, _I32, _P, _I64, _P,
                                              _P, _P]),
    "tfgx_nbr_static_input_hop_h16": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _I32, _I32, _P, _I32, _P, _I64, _I64, _I32, _I32, _P,
                                                     _I64, _P, _P, _P]),
    "tfgx_gather_rows_h16_f32": (ctypes.c_int, [_P, _I64, _I32, _P, _I64, _I64, _P, _I64, _P]),
}

# include/tfgx_collate_static.h (fixed-shape batches: device-resident ids, capacities the host knows, no reads)
COLLATE_STATIC_ABI_VERSION = 1
COLLATE_STATIC_DEAD = -1             # TFGX_STATIC_BATCH_DEAD: a dead slot of the id list
COLLATE_STATIC_BAD_ID, COLLATE_STATIC_OVERFLOW = 1, 2      # bits of counts[3]
COLLATE_STATIC_MAX_SLOTS = 1 << 20   # TFGX_STATIC_BATCH_MAX_SLOTS
COLLATE_STATIC_SIGNATURES = {
    "tfgx_static_batch_version": (ctypes.c_int, []),
    "tfgx_static_batch_table": (ctypes.c_int, [_P, _I64, _P, _P, _I64, _I64, _I64, _P, _P, _P, _P]),
    "tfgx_static_batch": (ctypes.c_int, [ctypes.POINTER(CollateStaticArgs), _P]),
}

class StaticPoolArgs(ctypes.Structure):
    """struct tfgx_static_pool_args (include/tfgx_pool_static.h)."""
    _fields_ = [
        ("row", ctypes.c_void_p), ("col", ctypes.c_void_p), ("w", ctypes.c_void_p), ("edge_graph_index", ctypes.c_void_p),
        ("n_cap", ctypes.c_int64), ("e_cap", ctypes.c_int64), ("B", ctypes.c_int64), ("sinks", ctypes.c_int64),
        ("sink_degree", ctypes.c_int64),
        ("node_map", ctypes.c_void_p), ("node_index", ctypes.c_void_p), ("pooled_row_ptr", ctypes.c_void_p),
        ("n_cap_out", ctypes.c_int64),
        ("out_row", ctypes.c_void_p), ("out_col", ctypes.c_void_p), ("out_edge_id", ctypes.c_void_p),
        ("out_edge_graph_index", ctypes.c_void_p), ("out_w", ctypes.c_void_p),
        ("plan", ctypes.POINTER(CollatePlan)), ("plan_t", ctypes.POINTER(CollatePlan)),
        ("counts", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


# include/tfgx_pool_static.h (one fixed-shape SAGPool level: static batch in, static batch out, no reads)
STATIC_POOL_ABI_VERSION = 1
STATIC_POOL_MAX_GRAPH_NODES = 4096   # TFGX_STATIC_POOL_MAX_GRAPH_NODES: the longest graph the selection ranks in LDS
STATIC_POOL_CLAMPED, STATIC_POOL_TOO_LONG = 4, 8      # bits of counts[3], beside the two of collate_static
STATIC_POOL_MAX_SLOTS = 1 << 20      # TFGX_STATIC_POOL_MAX_SLOTS
STATIC_POOL_SIGNATURES = {
    "tfgx_static_pool_version": (ctypes.c_int, []),
    "tfgx_static_pool_table": (ctypes.c_int, [_P, _P, _I64, _I32, _F32, _I64, _I64, _P, _P, _P]),
    "tfgx_static_pool_select": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _I64, _I64, _P, _P, _P, _P]),
    "tfgx_static_pool_edges_workspace_bytes": (_SZ, [_I64, _I64]),
    "tfgx_static_pool_edges": (ctypes.c_int, [ctypes.POINTER(StaticPoolArgs), _P]),
    "tfgx_static_pool_gather_scale_rows_f32": (ctypes.c_int, [_P, _I64, _I64, _P, _P, _I64, _I64, _P, _I64, _P]),
}

# include/tfgx_rows3d.h (node rows -> the dense [G, k, F] tensor: convert_x_to_3d and the fused SortPool readout, one launch)
ROWS3D_ABI_VERSION = 1
ROWS3D_TOO_LONG = STATIC_POOL_TOO_LONG      # TFGX_ROWS3D_TOO_LONG: the flag word of a sort-mode call, ORed into counts[3]
ROWS3D_MAX_GRAPH_NODES = STATIC_POOL_MAX_GRAPH_NODES      # the longest graph the sort mode ranks in LDS
ROWS3D_SIGNATURES = {
    "tfgx_rows3d_version": (ctypes.c_int, []),
    "tfgx_segment_rows_3d_f32": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _P, _I64, _P, _I64, _P, _P, _P, _P]),
}

class DensePoolStaticArgs(ctypes.Structure):
    """struct tfgx_dense_pool_static_args (include/tfgx_dense_pool_static.h)."""
    _fields_ = [
        ("P", ctypes.c_void_p), ("ldp", ctypes.c_int64), ("graph_mask", ctypes.c_void_p), ("parent_counts", ctypes.c_void_p),
        ("B", ctypes.c_int64), ("K", ctypes.c_int64), ("drop_diagonal", ctypes.c_int32),
        ("n_cap_out", ctypes.c_int64), ("e_cap", ctypes.c_int64), ("sinks", ctypes.c_int64), ("sink_degree", ctypes.c_int64),
        ("pooled_row_ptr", ctypes.c_void_p), ("node_index", ctypes.c_void_p), ("node_graph_index", ctypes.c_void_p),
        ("node_map", ctypes.c_void_p),
        ("out_row", ctypes.c_void_p), ("out_col", ctypes.c_void_p), ("out_edge_src", ctypes.c_void_p),
        ("out_edge_graph_index", ctypes.c_void_p),
        ("plan", ctypes.POINTER(CollatePlan)), ("plan_t", ctypes.POINTER(CollatePlan)),
        ("counts", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


# include/tfgx_dense_pool_static.h (the pooled batch of one fixed-shape DiffPool / MinCutPool level: S^T A S blocks in, static batch out)
DENSE_POOL_STATIC_ABI_VERSION = 1
DENSE_POOL_STATIC_MAX_K = 64             # TFGX_DENSE_POOL_STATIC_MAX_K: TFGX_SEGGRAM_MAX_K, a row of a block is one wave ballot
DENSE_POOL_STATIC_MAX_SLOTS = 1 << 20    # TFGX_DENSE_POOL_STATIC_MAX_SLOTS
DENSE_POOL_STATIC_SIGNATURES = {
    "tfgx_dense_pool_static_version": (ctypes.c_int, []),
    "tfgx_dense_pool_static_workspace_bytes": (_SZ, [_I64]),
    "tfgx_dense_pool_static": (ctypes.c_int, [ctypes.POINTER(DensePoolStaticArgs), _P]),
}

class AsapStaticEdgesArgs(ctypes.Structure):
    """struct tfgx_asapstatic_edges_args (include/tfgx_asap_static.h)."""
    _fields_ = [
        ("P", ctypes.c_void_p), ("ldp", ctypes.c_int64), ("pooled_row_ptr", ctypes.c_void_p),
        ("B", ctypes.c_int64), ("K", ctypes.c_int64),
        ("n_cap_out", ctypes.c_int64), ("e_cap", ctypes.c_int64), ("sinks", ctypes.c_int64), ("sink_degree", ctypes.c_int64),
        ("out_row", ctypes.c_void_p), ("out_col", ctypes.c_void_p), ("out_edge_src", ctypes.c_void_p),
        ("out_edge_graph_index", ctypes.c_void_p),
        ("plan", ctypes.POINTER(CollatePlan)), ("plan_t", ctypes.POINTER(CollatePlan)),
        ("counts", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


# include/tfgx_asap_static.h (one fixed-shape ASAP level: attention with absent self-loops, the dense assignment, the ragged
# pooled edge list with both plans)
ASAPSTATIC_ABI_VERSION = 1
ASAPSTATIC_MAX_K = 64                    # TFGX_ASAPSTATIC_MAX_K: TFGX_SEGGRAM_MAX_K, a row of a block is one wave ballot
ASAPSTATIC_MAX_FEATURES = 256            # TFGX_ASAPSTATIC_MAX_FEATURES: TFGX_ASAP_MAX_FEATURES, the same kernel
ASAPSTATIC_MAX_SLOTS = 1 << 20           # TFGX_ASAPSTATIC_MAX_SLOTS
ASAPSTATIC_SIGNATURES = {
    "tfgx_asapstatic_version": (ctypes.c_int, []),
    "tfgx_asapstatic_attend_f32": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _I64, _I64, _P, _P, _P, _F32, _U64, _P, _I32, _P, _I64, _P,
                                                  _P, _P, _P, _P, _P]),
    "tfgx_asapstatic_attend_backward_f32": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _P, _P, _P,
                                                           _P]),
    "tfgx_asapstatic_assign_f32": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _P, _I32, _P, _P, _P, _I64, _I64, _I64, _P, _I64, _P]),
    "tfgx_asapstatic_edges_workspace_bytes": (_SZ, [_I64]),
    "tfgx_asapstatic_edges": (ctypes.c_int, [ctypes.POINTER(AsapStaticEdgesArgs), _P]),
}

# One record per header under include/, tfgx.h first: the file, its version function with the version bound here, its table, and
# the (function, value) pairs of the constants the library was built with.  bind() and tests/test_abi_registry.py walk this
# registry; a new header is one more entry ("Adding a header").
Abi = collections.namedtuple("Abi", "header version_fn version signatures constants")
ABIS = (
    Abi("tfgx.h", "tfgx_version", ABI_VERSION, SIGNATURES, ()),
    Abi("tfgx_h16.h", "tfgx_h16_version", H16_ABI_VERSION, H16_SIGNATURES, ()),
    Abi("tfgx_fused_h16.h", "tfgx_fused_h16_version", FUSED_H16_ABI_VERSION, FUSED_H16_SIGNATURES, ()),
    Abi("tfgx_gemm_h16.h", "tfgx_gemm_h16_version", GEMM_H16_ABI_VERSION, GEMM_H16_SIGNATURES, ()),
    Abi("tfgx_dropedge.h", "tfgx_dropedge_version", DROPEDGE_ABI_VERSION, DROPEDGE_SIGNATURES, ()),
    Abi("tfgx_linkpred.h", "tfgx_linkpred_version", LINKPRED_ABI_VERSION, LINKPRED_SIGNATURES, ()),
    Abi("tfgx_lstm.h", "tfgx_lstm_version", LSTM_ABI_VERSION, LSTM_SIGNATURES, ()),
    Abi("tfgx_set2set.h", "tfgx_set2set_version", SET2SET_ABI_VERSION, SET2SET_SIGNATURES, ()),
    Abi("tfgx_asap.h", "tfgx_asap_version", ASAP_ABI_VERSION, ASAP_SIGNATURES, ()),
    Abi("tfgx_seggram.h", "tfgx_seggram_version", SEGGRAM_ABI_VERSION, SEGGRAM_SIGNATURES, (("tfgx_seggram_block", SEGGRAM_BLOCK),)),
    Abi("tfgx_normgrad.h", "tfgx_normgrad_version", NORMGRAD_ABI_VERSION, NORMGRAD_SIGNATURES, ()),
    Abi("tfgx_collate.h", "tfgx_collate_version", COLLATE_ABI_VERSION, COLLATE_SIGNATURES, (("tfgx_collate_tile", COLLATE_TILE),)),
    Abi("tfgx_nbrblock.h", "tfgx_nbrblock_version", NBRBLOCK_ABI_VERSION, NBRBLOCK_SIGNATURES, ()),
    Abi("tfgx_samplereduce.h", "tfgx_samplereduce_version", SAMPLEREDUCE_ABI_VERSION, SAMPLEREDUCE_SIGNATURES, ()),
    Abi("tfgx_nbrstatic.h", "tfgx_nbrstatic_version", NBRSTATIC_ABI_VERSION, NBRSTATIC_SIGNATURES, ()),
    Abi("tfgx_minibatch_h16.h", "tfgx_minibatch_h16_version", MINIBATCH_H16_ABI_VERSION, MINIBATCH_H16_SIGNATURES, ()),
    Abi("tfgx_collate_static.h", "tfgx_static_batch_version", COLLATE_STATIC_ABI_VERSION, COLLATE_STATIC_SIGNATURES, ()),
    Abi("tfgx_pool_static.h", "tfgx_static_pool_version", STATIC_POOL_ABI_VERSION, STATIC_POOL_SIGNATURES, ()),
    Abi("tfgx_rows3d.h", "tfgx_rows3d_version", ROWS3D_ABI_VERSION, ROWS3D_SIGNATURES, ()),
    Abi("tfgx_dense_pool_static.h", "tfgx_dense_pool_static_version", DENSE_POOL_STATIC_ABI_VERSION, DENSE_POOL_STATIC_SIGNATURES, ()),
    Abi("tfgx_asap_static.h", "tfgx_asapstatic_version", ASAPSTATIC_ABI_VERSION, ASAPSTATIC_SIGNATURES, ()),
)

# C struct name -> its ctypes mirror: every ctypes.Structure of this module
STRUCTS = {
    "tfgx_reduce_args": ReduceArgs, "tfgx_gat_args": GatArgs, "tfgx_hub_lists": HubLists,
    "tfgx_gat_backward_args": GatBackwardArgs, "tfgx_drop_edge_plan": DropEdgePlan, "tfgx_collate_plan": CollatePlan,
    "tfgx_collate_args": CollateArgs, "tfgx_static_batch_args": CollateStaticArgs,
    "tfgx_static_pool_args": StaticPoolArgs, "tfgx_dense_pool_static_args": DensePoolStaticArgs,
    "tfgx_asapstatic_edges_args": AsapStaticEdgesArgs,
}


def bind(lib, abis=ABIS):
    """Set restype / argtypes of every table of `abis` on `lib` (a ctypes.CDLL), then compare what the library was built with
    against what this package binds: each header's version and each of its constants.  Returns lib."""
    for abi in abis:
        for name, (res, args) in abi.signatures.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
    for abi in abis:
        for name, bound in ((abi.version_fn, abi.version),) + tuple(abi.constants):
            built = getattr(lib, name)()
            if built != bound:
                raise TfgxError("tf_geometric_amd: {} was built with {}() = {} but this package binds {} (include/{}): "
                                "rebuild with __graft_entry__.build()".format(lib._name, name, built, bound, abi.header))
    return lib


_lib = None


def load_library():
    """Load libtfgx.so and bind() every header of ABIS. Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH) and os.path.exists("/opt/rocm/bin/hipcc"):
        try:     # sources are in-tree: build once (hipcc --offload-arch=gfx950, ~15 s); never a CPU fallback
            from . import _build
            _build.build(verbose=False)
        except Exception as ex:      # noqa: BLE001 - reported below with the build hint
            raise TfgxError("tf_geometric_amd: building {} failed: {}".format(LIB_PATH, ex))
    if not os.path.exists(LIB_PATH):
        raise TfgxError(
            "tf_geometric_amd: HIP library {} is missing. Build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.".format(LIB_PATH))
    _lib = bind(ctypes.CDLL(LIB_PATH))
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = load_library().tfgx_last_error()
        raise TfgxError("{} failed with code {}: {}".format(what or "tfgx call", rc, (msg or b"").decode()))


def require_gpu():
    if not torch.cuda.is_available():
        raise TfgxError("tf_geometric_amd needs an AMD GPU (gfx950 / MI355X); torch.cuda.is_available() is False "
                        "and there is no CPU fallback.")
    return load_library()


def device():
    require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def as_f32(x, dev=None):
    """numpy / list / torch -> contiguous float32 tensor on the GPU (float64 is down-cast as data/graph.py:79-86)."""
    dev = dev or device()
    if isinstance(x, torch.Tensor):
        # keep the autograd edge of tensors that are being trained (autograd.py); plain inputs are detached
        t = x if (x.requires_grad and torch.is_grad_enabled()) else x.detach()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.device != dev:
        t = t.to(dev)
    if t.dim() >= 2 and t.stride(-1) != 1:
        t = t.contiguous()
    if t.dim() == 1 and not t.is_contiguous():
        t = t.contiguous()
    return t


def as_i32(x, dev=None):
    dev = dev or device()
    if isinstance(x, torch.Tensor):
        t = x.detach()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if t.dtype != torch.int32:
        t = t.to(torch.int32)          # data/graph.py:59-66: edge_index is cast to int32
    if t.device != dev:
        t = t.to(dev)
    return t.contiguous()


def row_major_2d(t):
    """Return (tensor, leading dimension) for a 2-D float32 tensor whose rows are dense."""
    assert t.dim() == 2
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    ld = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)
    return t, ld
