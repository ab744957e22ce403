// The two gathers more than one source launches.  Kernel templates: each .hip file instantiates what it launches.
#pragma once
#include "tfgx_common.h"

namespace tfgx {

// dst[i] = src[idx[i]]
template <class T>
__global__ void gather_by_index(const T* __restrict__ src, const int32_t* __restrict__ idx, int64_t n, T* __restrict__ dst)
{
    int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; i < n; i += stride) dst[i] = src[idx[i]];
}

// out[i, :] = x[idx[i], :] * s[idx[i]] (s == NULL: plain gather).  Row i = F4 float4 items + (F - 4 F4) scalar tail items.
// CLAMPED: out[i, :] = 0 where idx[i] is outside [0, n).  The load is clamped (row max(idx, 0), below n), the zero is a select.
template <bool CLAMPED>
__global__ void gather_scale_rows(const float* __restrict__ x, int64_t ldx, int64_t n, const int32_t* __restrict__ idx,
                                  const float* __restrict__ s, int64_t M, int64_t F, int64_t F4, float* __restrict__ out,
                                  int64_t ldo)
{
    const int64_t W = F4 + (F - 4 * F4);
    const int64_t total = M * W;
    int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; t < total; t += stride) {
        const int64_t i = t / W, q = t - i * W;
        const int32_t raw = idx[i];
        const bool live = !CLAMPED || (raw >= 0 && raw < n);
        const int64_t r = CLAMPED ? min(int64_t(max(raw, 0)), n - 1) : int64_t(raw);
        const float sc = s != nullptr ? s[r] : 1.0f;
        if (q < F4) {
            float v[4];
            load_vec<4>(x + r * ldx + 4 * q, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = live ? v[k] * sc : 0.0f;
            store_vec<4>(out + i * ldo + 4 * q, v);
        } else {
            const int64_t c = 4 * F4 + (q - F4);
            const float v = x[r * ldx + c] * sc;
            out[i * ldo + c] = live ? v : 0.0f;
        }
    }
}

}  // namespace tfgx
