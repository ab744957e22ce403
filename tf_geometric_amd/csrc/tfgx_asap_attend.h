// ASAP's fused 1-hop attention forward, the ONE implementation behind tfgx_asap_attend_f32 (include/tfgx_asap.h) and
// tfgx_asapstatic_attend_f32 (include/tfgx_asap_static.h).
//
// A WAVE owns one destination row.  It walks the row 64 edges at a time: lane l scores edge pos + l (two scalar gathers), the
// chunk's maximum and sum meet in xor trees, then the chunk's edges are taken one by one (their column and weight broadcast from
// the owning lane) with the lanes spread over the feature columns, 64 apart, up to four per lane.  The running state is
// (m, l, acc): m the maximum so far, l the sum of exp(s - m) over every edge EXCEPT the one that set m (its 1 is added where the
// denominator is used), acc the un-normalised feature sum.  A second walk over the row's scalars writes the normalised weights.
// The trees depend on nothing but the lane count, so the bits do not depend on scheduling.
//
// SKIP_LOOPS (the fixed-shape route): an edge with col == its row is absent — it scores -inf, weighs 0, reads nothing and gets
// p = p_drop = 0.  It is NOT a bad edge.  The flag is a template parameter: SKIP_LOOPS = false compiles to the kernel that was
// here before, and on a list without self-loops both instantiations execute the same arithmetic on the same operands.
#pragma once
#include "tfgx_common.h"

namespace tfgx {
namespace asap_attend {

constexpr int kWaves = kBlock / kWave;
constexpr float kEps = 1e-8f;
constexpr float kAlpha = 0.2f;

__device__ __forceinline__ float leaky(float z) { return z > 0.0f ? z : kAlpha * z; }

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// T = feature columns per lane (F <= 64 T)
template <int T, bool SKIP_LOOPS>
__global__ void __launch_bounds__(kBlock) kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, int64_t N,
                                                 int64_t E, const float* __restrict__ x, int64_t ldx, int F,
                                                 const float* __restrict__ sq, const float* __restrict__ sh,
                                                 const float* __restrict__ bias, DropCfg drop, float* __restrict__ c, int64_t ldc,
                                                 float* __restrict__ p, float* __restrict__ p_self, float* __restrict__ p_drop,
                                                 float* __restrict__ p_self_drop, int32_t* __restrict__ flag)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const float b0 = *bias;
    int bad = 0;
    for (int64_t row = int64_t(blockIdx.x) * kWaves + wave; row < N; row += int64_t(gridDim.x) * kWaves) {
        int64_t beg = row_ptr[row], end = row_ptr[row + 1];
        if (!(beg >= 0 && end >= beg && end <= E)) {
            bad = 1;
            beg = end = 0;
        }
        const float sqr = sq[row] + b0;
        const float s_self = leaky(sqr + sh[row]);
        const float k_self = drop_scale(drop, uint32_t(E + row));
        float m = s_self, l = 0.0f;
        float acc[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int f = lane + 64 * t;
            acc[t] = (f < F && k_self != 0.0f) ? k_self * x[row * ldx + f] : 0.0f;
        }
        for (int64_t pos = beg; pos < end; pos += kWave) {
            const int64_t i = pos + lane;
            const bool act = i < end;
            const int32_t cj = act ? col[i] : 0;
            const bool valid = act && cj >= 0 && int64_t(cj) < N;
            if (act && !valid) bad = 1;
            const bool ok = valid && !(SKIP_LOOPS && int64_t(cj) == row);
            const float s = ok ? leaky(sqr + sh[cj]) : -INFINITY;
            const float mc = wave_max(s);
            int owner = -1;
            if (mc > m) {      // wave-uniform
                const float scale = expf(m - mc);
                l = (l + 1.0f) * scale;      // the old maximum's own 1 becomes an ordinary term
#pragma unroll
                for (int t = 0; t < T; ++t) acc[t] *= scale;
                m = mc;
                owner = __ffsll(static_cast<unsigned long long>(__ballot(s == mc))) - 1;
            }
            const float ex = ok ? expf(s - m) : 0.0f;
            l += wave_sum(lane == owner ? 0.0f : ex);      // the chunk is summed first, then folded into l
            const float wgt = ok ? ex * drop_scale(drop, uint32_t(i)) : 0.0f;
            const int cnt = int(end - pos < kWave ? end - pos : kWave);
            for (int k = 0; k < cnt; ++k) {
                const float wk = __shfl(wgt, k);
                const int32_t ck = __shfl(cj, k);
                if (wk != 0.0f) {      // wave-uniform: a dropped (or invalid, or absent) edge reads nothing
                    const float* __restrict__ xr = x + int64_t(ck) * ldx;
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const int f = lane + 64 * t;
                        if (f < F) acc[t] += wk * xr[f];
                    }
                }
            }
        }
        const float D = (l + 1.0f) + kEps;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int f = lane + 64 * t;
            if (f < F) c[row * ldc + f] = acc[t] / D;
        }
        if (lane == 0) {
            const float ps = expf(s_self - m) / D;
            p_self[row] = ps;
            if (p_self_drop != nullptr) p_self_drop[row] = ps * k_self;
        }
        for (int64_t i = beg + lane; i < end; i += kWave) {
            const int32_t cj = col[i];
            const bool ok = cj >= 0 && int64_t(cj) < N && !(SKIP_LOOPS && int64_t(cj) == row);
            const float pe = ok ? expf(leaky(sqr + sh[ok ? cj : 0]) - m) / D : 0.0f;
            p[i] = pe;
            if (p_drop != nullptr) p_drop[i] = pe * drop_scale(drop, uint32_t(i));
        }
    }
    if (flag != nullptr && __any(bad) && lane == 0) atomicOr(flag, 1);
}

// The launch both entry points share, after their own argument checks.  N > 0.
template <bool SKIP_LOOPS>
inline void launch(const int32_t* row_ptr, const int32_t* col, int64_t N, int64_t E, const float* x, int64_t ldx, int64_t F,
                   const float* sq, const float* sh, const float* bias, const DropCfg& drop, float* c, int64_t ldc, float* p,
                   float* p_self, float* p_drop, float* p_self_drop, int32_t* bad_flag, hipStream_t stream)
{
    const int grid = grid_for(N, kWaves);
    const int f = int(F);
#define TFGX_ASAP_LAUNCH(T)                                                                                                      \
    kernel<T, SKIP_LOOPS><<<grid, kBlock, 0, stream>>>(row_ptr, col, N, E, x, ldx, f, sq, sh, bias, drop, c, ldc, p, p_self,    \
                                                       p_drop, p_self_drop, bad_flag)
    if (f <= 64) TFGX_ASAP_LAUNCH(1);
    else if (f <= 128) TFGX_ASAP_LAUNCH(2);
    else if (f <= 192) TFGX_ASAP_LAUNCH(3);
    else TFGX_ASAP_LAUNCH(4);
#undef TFGX_ASAP_LAUNCH
}

}  // namespace asap_attend
}  // namespace tfgx
