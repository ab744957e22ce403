# coding=utf-8
"""tf_geometric_amd — MI355X (gfx950) message-passing backend behind tf_geometric's own API.

    import tf_geometric_amd as tfg
    h = tfg.layers.GCN(16, activation=tfg.relu)([x, edge_index, edge_weight], cache=graph_cache)

Only the hot path of the reference is here: aggregate_neighbors / GCN / GAT / GraphSAGE,
the dense x @ W next to it, and dst-range sharding with halo exchange.  Compute = hand-written HIP kernels in
lib/libtfgx.so (C ABI: include/tfgx.h); importing works without a GPU, calling an operator does not.
"""
import torch as _torch

from . import _lib
from .activations import relu
from .plan import CsrPlan, prepare_static_features, release_static_features, HalfRows
from .sparse import SparseMatrix
from . import nn
from . import layers
from . import dist
from . import utils
from . import data
from .data import Graph, BatchGraph
from .graph_capture import CapturedForward, CapturedTrainStep


def prepare_half_features(x, dtype=_torch.bfloat16, gemm_operand=False, ld=None, minibatch=False):
    """Store a float32 feature table in 16 bits (torch.bfloat16 by default, or torch.float16) for the aggregation kernels:
    a HalfRows on the line-friendly row stride (or on `ld` elements), quantised by tfgx_rows_f32_to_h16 (round to nearest
    even).  Arithmetic stays float32; the result of every reduce over it equals the float32 route's on
    half_features_to_f32(h) bit for bit.

    gemm_operand=True also declares the table for the GEMM position: GCN with units <= num_features, GAT and the mean / sum
    GraphSAGE layers then read it in their projections and weight gradients (include/tfgx_gemm_h16.h) — the float32 layer's
    bits on half_features_to_f32(h), outputs and parameter gradients, with no widened [N, F] copy.  The flag is the caller's
    choice and nothing falls back to a widened copy behind it.  Measured (tools/bench_gemm_half.py): on no
    shape is reading the table behind widening it first (1.25x to 7x ahead); against a float32 copy that is already held, the
    narrow-output (skinny) route is 34-38 % faster, the row kernel level, and the LDS-staged kernel slower — 233 k x 602 -> 64
    by 22 %, -> 256 by 7 %.

    minibatch=True declares the table for the minibatch route (include/tfgx_minibatch_h16.h): RandomNeighborSampler.sample_reduce
    and the gather / input_aggregate of SampledMinibatch and StaticMinibatch then read it in place and return float32 rows — the
    float32 route's bits on half_features_to_f32(h), with no float32 copy of the table.  Without the flag they refuse it."""
    return HalfRows.from_dense(x, dtype=dtype, ld=ld, gemm_operand=gemm_operand, minibatch=minibatch)


def half_features_to_f32(h):
    """The dense float32 [n, F] tensor a HalfRows stands for (exact)."""
    return h.float()


__version__ = "0.1.0"
