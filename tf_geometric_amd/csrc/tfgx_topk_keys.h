// The score key of top-k selection, shared by tfgx_topk.hip (global radix sort) and tfgx_pool_static.hip (per-graph selection in
// LDS): both order nodes by the same 32 bits, so both select the same nodes.
#pragma once
#include "tfgx_common.h"

namespace tfgx {

// ascending unsigned order of the result == DESCENDING float order; -0.0 and +0.0 compare equal (as in top_k)
__device__ __forceinline__ uint32_t descending_bits(float f)
{
    uint32_t u = __float_as_uint(f == 0.0f ? 0.0f : f);
    u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;   // order-preserving map of IEEE-754 onto unsigned
    return ~u;
}

// node_k (tf_geometric/nn/pool/topk_pool.py:62-71): min(k, count), or ceil(float32(count) * float32(ratio)) — clamped to count,
// where the reference would start selecting its padding columns for ratio > 1.  k >= 0 selects the first form.
__device__ __forceinline__ int32_t topk_node_k(int32_t cnt, int32_t k, float ratio)
{
    return (k >= 0) ? min(k, cnt) : min(cnt, int32_t(ceilf(float(cnt) * ratio)));
}

}  // namespace tfgx
