// The LSTM aggregator of GraphSAGE (include/tfgx_lstm.h): fused gather -> recurrence, and its backward through time.
//
// Reference: nn/conv/graph_sage.py:290-356 (a dense [N, T, F] gather + a Keras LSTM + reduce_mean over the T steps).
//
// One workgroup (4 waves) owns kTile = 32 destination rows for all T steps.  The recurrent product h @ R ([32, U] x [U, 4U])
// runs on v_mfma_f32_16x16x4_f32: wave w owns the 16-unit blocks jb = w, w + 4, ... and for each of them the FOUR gate
// column blocks (jb * 16 + g * U), so the lane that holds unit u of row r in the MFMA's D layout (col = lane & 15,
// row = 4 (lane >> 4) + reg) holds all four pre-activations of (r, u): the gates, c and sum_t h_t never leave its registers.
// h_t goes through a [32][U + 2] LDS tile (the A operand of the next step; the + 2 makes the 16 rows x 2 k of a
// ds_read_b32 lane group hit 32 distinct banks).  R is LDS-resident when it fits beside that tile — columns of odd k rows
// are stored xor 16 so that the two k rows of a lane group fall into different bank halves — and otherwise read from L2
// straight into the B operand: with a 32-row tile an element of R feeds exactly two MFMAs per step, so a hop through LDS
// would add traffic, not reuse.
//
// Backward: the same tiling, t = T-1 .. 0.  The pointwise part rebuilds dz from the saved gates and c, writes it to HBM and to
// a [32][4U + 2] LDS tile, which is the A operand of dh_{t-1} = dz_t @ R^T (B = R^T, LDS-resident as [4U][U] when it fits).
#include "tfgx_common.h"
#include "../../include/tfgx_lstm.h"

namespace tfgx {
namespace {

constexpr int kTile = TFGX_LSTM_TILE_ROWS;      // rows per workgroup = 2 MFMA row tiles
constexpr int kRowTiles = kTile / 16;
constexpr int kMaxBlocksPerWave = TFGX_LSTM_MAX_UNITS / 16 / (kBlock / kWave);     // 4
constexpr size_t kLdsLimit = 160 * 1024;
constexpr int64_t kInt32Max = (int64_t(1) << 31) - 1;

typedef float f32x4 __attribute__((ext_vector_type(4)));

inline size_t fwd_lds_bytes(int64_t U, bool resident)
{
    return sizeof(float) * (size_t(kTile) * size_t(U + 2) + (resident ? size_t(U) * size_t(4 * U) : 0));
}
inline size_t bwd_lds_bytes(int64_t U, bool resident)
{
    return sizeof(float) * (size_t(kTile) * size_t(4 * U + 2) + (resident ? size_t(U) * size_t(4 * U) : 0));
}
inline bool units_ok(int64_t U) { return U >= 16 && U <= TFGX_LSTM_MAX_UNITS && U % 16 == 0; }

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// saved state of (row i, step t): 5U floats at ((i * T + t) * 5U): the activated gates i, f, g, o (U each), then c_t.
template <bool RES, bool SAVE>
__global__ void __launch_bounds__(kBlock) lstm_forward_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                              int64_t n_dst, int64_t n_src, int T, const float* __restrict__ P,
                                                              int64_t ldp, const float* __restrict__ p_pad,
                                                              const float* __restrict__ R, int U, float* __restrict__ out,
                                                              int64_t ldo, float* __restrict__ saved, int32_t* __restrict__ flag)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int ldh = U + 2, N4 = 4 * U, nb = U / 16;
    float* hs = lds;                    // [kTile][ldh]
    float* Rs = lds + kTile * ldh;      // [U][4U], column ^ 16 on odd k (RES only)
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, l15 = lane & 15, kq = lane >> 4;
    const int swz = (kq & 1) << 4;
    const int64_t row0 = int64_t(blockIdx.x) * kTile;

    if constexpr (RES) {
        for (int idx = tid; idx < U * N4; idx += kBlock) {
            const int k = idx / N4, c = idx - k * N4;
            Rs[k * N4 + (c ^ ((k & 1) << 4))] = R[idx];
        }
    }
    for (int idx = tid; idx < kTile * ldh; idx += kBlock) hs[idx] = 0.0f;

    int beg[kRowTiles][4], deg[kRowTiles][4];
    int bad = 0;
#pragma unroll
    for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t gi = row0 + rt * 16 + kq * 4 + r;
            int b = 0, d = 0;
            if (gi < n_dst) {
                b = row_ptr[gi];
                const int64_t dd = int64_t(row_ptr[gi + 1]) - b;
                bad |= (dd < 0) | (dd > T) | (b < 0);
                d = dd < 0 || b < 0 ? 0 : (dd > T ? T : int(dd));
            }
            beg[rt][r] = b;
            deg[rt][r] = d;
        }

    float c[kMaxBlocksPerWave][kRowTiles][4], hsum[kMaxBlocksPerWave][kRowTiles][4], hn[kMaxBlocksPerWave][kRowTiles][4];
#pragma unroll
    for (int q = 0; q < kMaxBlocksPerWave; ++q)
#pragma unroll
        for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) c[q][rt][r] = hsum[q][rt][r] = hn[q][rt][r] = 0.0f;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const float* pp[kRowTiles][4];
#pragma unroll
        for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* p = p_pad;
                if (t < deg[rt][r]) {
                    const int32_t j = col[int64_t(beg[rt][r]) + t];
                    const bool ok = (j >= 0) & (int64_t(j) < n_src);
                    bad |= !ok;
                    if (ok) p = P + int64_t(j) * ldp;
                }
                pp[rt][r] = p;
            }
#pragma unroll
        for (int q = 0; q < kMaxBlocksPerWave; ++q) {
            const int jb = wave + q * (kBlock / kWave);
            if (jb < nb) {
                const int u = jb * 16 + l15;
                // the gathered rows of this block: issued before the MFMA chain, consumed after it
                float pv[kRowTiles][4][4];
#pragma unroll
                for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int g = 0; g < 4; ++g) pv[rt][r][g] = pp[rt][r][g * U + u];
                f32x4 acc[kRowTiles][4];
#pragma unroll
                for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[rt][g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (t > 0) {        // h_0 = 0: the first step has no recurrent term
                    for (int k0 = 0; k0 < U; k0 += 4) {
                        const int k = k0 + kq;
                        float a[kRowTiles];
#pragma unroll
                        for (int rt = 0; rt < kRowTiles; ++rt) a[rt] = hs[(rt * 16 + l15) * ldh + k];
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int cc = g * U + u;
                            const float b = RES ? Rs[k * N4 + (cc ^ swz)] : R[int64_t(k) * N4 + cc];
#pragma unroll
                            for (int rt = 0; rt < kRowTiles; ++rt)
                                acc[rt][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt], b, acc[rt][g], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float gi_ = sigmoidf_(acc[rt][0][r] + pv[rt][r][0]);
                        const float gf = sigmoidf_(acc[rt][1][r] + pv[rt][r][1]);
                        const float gg = tanhf(acc[rt][2][r] + pv[rt][r][2]);
                        const float go = sigmoidf_(acc[rt][3][r] + pv[rt][r][3]);
                        const float cn = gf * c[q][rt][r] + gi_ * gg;
                        const float h = go * tanhf(cn);
                        c[q][rt][r] = cn;
                        hn[q][rt][r] = h;
                        hsum[q][rt][r] += h;
                        if constexpr (SAVE) {
                            const int64_t gi = row0 + rt * 16 + kq * 4 + r;
                            if (gi < n_dst) {
                                float* s = saved + (gi * T + t) * int64_t(5 * U) + u;
                                s[0] = gi_;
                                s[U] = gf;
                                s[2 * U] = gg;
                                s[3 * U] = go;
                                s[4 * U] = cn;
                            }
                        }
                    }
            }
        }
        __syncthreads();        // every wave has read h_{t-1}
#pragma unroll
        for (int q = 0; q < kMaxBlocksPerWave; ++q) {
            const int jb = wave + q * (kBlock / kWave);
            if (jb < nb) {
#pragma unroll
                for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) hs[(rt * 16 + kq * 4 + r) * ldh + jb * 16 + l15] = hn[q][rt][r];
            }
        }
        __syncthreads();
    }

    const float tf = float(T);
#pragma unroll
    for (int q = 0; q < kMaxBlocksPerWave; ++q) {
        const int jb = wave + q * (kBlock / kWave);
        if (jb < nb) {
#pragma unroll
            for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t gi = row0 + rt * 16 + kq * 4 + r;
                    if (gi < n_dst) out[gi * ldo + jb * 16 + l15] = hsum[q][rt][r] / tf;
                }
        }
    }
    if (flag != nullptr && __any(bad) && lane == 0) atomicOr(flag, 1);
}

template <bool RES>
__global__ void __launch_bounds__(kBlock) lstm_backward_kernel(const int32_t* __restrict__ row_ptr, int64_t n_dst, int T, int U,
                                                               const float* __restrict__ R, const float* __restrict__ d_mean,
                                                               int64_t ldd, const float* __restrict__ saved,
                                                               float* __restrict__ d_gates, float* __restrict__ h_prev,
                                                               float* __restrict__ d_pad_partial)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int N4 = 4 * U, ldz = N4 + 2, nb = U / 16;
    float* dzs = lds;                   // [kTile][ldz]
    float* Rt = lds + kTile * ldz;      // [4U][U] = R^T, column ^ 16 on odd k when U % 32 == 0 (RES only)
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, l15 = lane & 15, kq = lane >> 4;
    const int swz_on = (U % 32 == 0) ? 16 : 0;      // U % 32 == 16: consecutive k rows are 16 banks apart already
    const int swz = (kq & 1) ? swz_on : 0;
    const int64_t row0 = int64_t(blockIdx.x) * kTile;

    if constexpr (RES) {
        for (int idx = tid; idx < U * N4; idx += kBlock) {
            const int u = idx / N4, k = idx - u * N4;
            Rt[k * U + (u ^ ((k & 1) ? swz_on : 0))] = R[idx];
        }
    }

    int deg[kRowTiles][4];
#pragma unroll
    for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t gi = row0 + rt * 16 + kq * 4 + r;
            int d = 0;
            if (gi < n_dst) {
                const int b = row_ptr[gi];
                const int64_t dd = int64_t(row_ptr[gi + 1]) - b;
                d = dd < 0 || b < 0 ? 0 : (dd > T ? T : int(dd));
            }
            deg[rt][r] = d;
        }

    const float tf = float(T);
    float dm[kMaxBlocksPerWave][kRowTiles][4], dh_rec[kMaxBlocksPerWave][kRowTiles][4], dc_next[kMaxBlocksPerWave][kRowTiles][4];
    // a lane's pad sum runs over 8 rows x up to T steps, one term after the other: compensated (Kahan), or its rounding error
    // grows with T and passes that of the rest of the backward at T of a few dozen (hub rows of a pooled graph)
    float padacc[kMaxBlocksPerWave][4], padcmp[kMaxBlocksPerWave][4];
#pragma unroll
    for (int q = 0; q < kMaxBlocksPerWave; ++q) {
        const int jb = wave + q * (kBlock / kWave);
#pragma unroll
        for (int g = 0; g < 4; ++g) padacc[q][g] = padcmp[q][g] = 0.0f;
#pragma unroll
        for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t gi = row0 + rt * 16 + kq * 4 + r;
                dm[q][rt][r] = (jb < nb && gi < n_dst) ? d_mean[gi * ldd + jb * 16 + l15] / tf : 0.0f;
                dh_rec[q][rt][r] = 0.0f;
                dc_next[q][rt][r] = 0.0f;
            }
    }

    for (int t = T - 1; t >= 0; --t) {
#pragma unroll
        for (int q = 0; q < kMaxBlocksPerWave; ++q) {
            const int jb = wave + q * (kBlock / kWave);
            if (jb < nb) {
                const int u = jb * 16 + l15;
#pragma unroll
                for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int lr = rt * 16 + kq * 4 + r;
                        const int64_t gi = row0 + lr;
                        float dz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                        if (gi < n_dst) {
                            const int64_t it = gi * T + t;
                            const float* s = saved + it * int64_t(5 * U) + u;
                            const float gi_ = s[0], gf = s[U], gg = s[2 * U], go = s[3 * U], ct = s[4 * U];
                            float cp = 0.0f, hp = 0.0f;
                            if (t > 0) {
                                const float* sp = s - 5 * U;
                                cp = sp[4 * U];
                                hp = sp[3 * U] * tanhf(cp);
                            }
                            const float dh = dm[q][rt][r] + dh_rec[q][rt][r];
                            const float tc = tanhf(ct);
                            const float dc = dc_next[q][rt][r] + dh * go * (1.0f - tc * tc);
                            dz[0] = dc * gg * gi_ * (1.0f - gi_);
                            dz[1] = dc * cp * gf * (1.0f - gf);
                            dz[2] = dc * gi_ * (1.0f - gg * gg);
                            dz[3] = dh * tc * go * (1.0f - go);
                            dc_next[q][rt][r] = dc * gf;
                            float* dg = d_gates + it * int64_t(N4) + u;
#pragma unroll
                            for (int g = 0; g < 4; ++g) dg[g * U] = dz[g];
                            h_prev[it * int64_t(U) + u] = hp;
                            if (t >= deg[rt][r]) {
#pragma unroll
                                for (int g = 0; g < 4; ++g) {
                                    const float y = dz[g] - padcmp[q][g];
                                    const float sum = padacc[q][g] + y;
                                    padcmp[q][g] = (sum - padacc[q][g]) - y;
                                    padacc[q][g] = sum;
                                }
                            }
                        }
#pragma unroll
                        for (int g = 0; g < 4; ++g) dzs[lr * ldz + g * U + u] = dz[g];
                    }
            }
        }
        if (t == 0) break;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kMaxBlocksPerWave; ++q) {
            const int jb = wave + q * (kBlock / kWave);
            if (jb < nb) {
                const int u = jb * 16 + l15;
                f32x4 acc[kRowTiles][2];        // two chains over alternating k steps: the MFMA's latency exceeds its issue time
#pragma unroll
                for (int rt = 0; rt < kRowTiles; ++rt) acc[rt][0] = acc[rt][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                for (int k0 = 0; k0 < N4; k0 += 8) {
#pragma unroll
                    for (int ch = 0; ch < 2; ++ch) {
                        const int k = k0 + 4 * ch + kq;
                        const float b = RES ? Rt[k * U + (u ^ swz)] : R[int64_t(u) * N4 + k];
#pragma unroll
                        for (int rt = 0; rt < kRowTiles; ++rt)
                            acc[rt][ch] = __builtin_amdgcn_mfma_f32_16x16x4f32(dzs[(rt * 16 + l15) * ldz + k], b, acc[rt][ch], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dh_rec[q][rt][r] = acc[rt][0][r] + acc[rt][1][r];
            }
        }
        __syncthreads();
    }

    // the tile's pad sums: a lane holds its 8 rows' share; the four lane groups of a unit meet in a fixed xor tree
#pragma unroll
    for (int q = 0; q < kMaxBlocksPerWave; ++q) {
        const int jb = wave + q * (kBlock / kWave);
        if (jb < nb) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float v = padacc[q][g];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (kq == 0) d_pad_partial[int64_t(blockIdx.x) * N4 + g * U + jb * 16 + l15] = v;
            }
        }
    }
}

int check_common(const char* fn, int64_t n_dst, int64_t T, int64_t U)
{
    if (n_dst < 0 || T < 0 || U < 0) {
        set_error("%s: negative size (n_dst = %lld, T = %lld, U = %lld)", fn, (long long)n_dst, (long long)T, (long long)U);
        return TFGX_ERR_INVALID_ARG;
    }
    if (U != 0 && !units_ok(U)) {
        set_error("%s: U must be a multiple of 16 in [16, %d], got %lld", fn, TFGX_LSTM_MAX_UNITS, (long long)U);
        return TFGX_ERR_INVALID_ARG;
    }
    if (n_dst > kInt32Max || T > kInt32Max) {
        set_error("%s: n_dst and T must fit int32", fn);
        return TFGX_ERR_INVALID_ARG;
    }
    return TFGX_OK;
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_lstm_version(void) { return TFGX_LSTM_ABI_VERSION; }

extern "C" int tfgx_lstm_recurrent_kernel_resident(int64_t U, int32_t backward)
{
    if (!units_ok(U)) return 0;
    return (backward ? bwd_lds_bytes(U, true) : fwd_lds_bytes(U, true)) <= kLdsLimit ? 1 : 0;
}

extern "C" size_t tfgx_lstm_aggregate_saved_bytes(int64_t n_dst, int64_t T, int64_t U)
{
    if (n_dst <= 0 || T <= 0 || U <= 0) return 0;
    return size_t(n_dst) * size_t(T) * size_t(5 * U) * sizeof(float);
}

extern "C" int64_t tfgx_lstm_aggregate_tiles(int64_t n_dst) { return n_dst <= 0 ? 0 : (n_dst + kTile - 1) / kTile; }

extern "C" int tfgx_lstm_aggregate_f32(const int32_t* row_ptr, const int32_t* col, int64_t n_dst, int64_t n_src, int64_t T,
                                       const float* P, int64_t ldp, const float* p_pad, const float* R, int64_t U, float* out_mean,
                                       int64_t ldo, void* saved, size_t saved_bytes, int32_t* bad_flag, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_common(__func__, n_dst, T, U)) return rc;
    if (n_src < 0 || n_src > kInt32Max) {
        set_error("%s: n_src must be in [0, 2^31), got %lld", __func__, (long long)n_src);
        return TFGX_ERR_INVALID_ARG;
    }
    if (ldp < 4 * U || ldo < U) {
        set_error("%s: %s is too small (%lld < %lld)", __func__, ldp < 4 * U ? "ldp" : "ldo", (long long)(ldp < 4 * U ? ldp : ldo),
                  (long long)(ldp < 4 * U ? 4 * U : U));
        return TFGX_ERR_INVALID_ARG;
    }
    if (n_dst == 0 || U == 0) return TFGX_OK;
    if (out_mean == nullptr) {
        set_error("%s: out_mean is null", __func__);
        return TFGX_ERR_INVALID_ARG;
    }
    if (T == 0) {
        TFGX_HIP_CHECK(hipMemset2DAsync(out_mean, sizeof(float) * size_t(ldo), 0, sizeof(float) * size_t(U), size_t(n_dst), stream));
        return TFGX_OK;
    }
    if (row_ptr == nullptr || col == nullptr || p_pad == nullptr || R == nullptr) {
        set_error("%s: %s is null", __func__,
                  row_ptr == nullptr ? "row_ptr" : (col == nullptr ? "col" : (p_pad == nullptr ? "p_pad" : "R")));
        return TFGX_ERR_INVALID_ARG;
    }
    if (n_src > 0 && P == nullptr) {     // n_src == 0: every col is out of range, P is never read
        set_error("%s: P is null", __func__);
        return TFGX_ERR_INVALID_ARG;
    }
    if (saved != nullptr && saved_bytes < tfgx_lstm_aggregate_saved_bytes(n_dst, T, U)) {
        set_error("%s: saved_bytes is too small (%zu < %zu)", __func__, saved_bytes, tfgx_lstm_aggregate_saved_bytes(n_dst, T, U));
        return TFGX_ERR_INVALID_ARG;
    }
    const bool res = tfgx_lstm_recurrent_kernel_resident(U, 0) != 0;
    const size_t lds_bytes = fwd_lds_bytes(U, res);
    const int grid = int(tfgx_lstm_aggregate_tiles(n_dst));
#define TFGX_LSTM_FWD(RES_, SAVE_)                                                                                              \
    do {                                                                                                                        \
        static bool attr_set = false;                                                                                           \
        if (!attr_set) {                                                                                                        \
            TFGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_forward_kernel<RES_, SAVE_>),                 \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, int(kLdsLimit)));                    \
            attr_set = true;                                                                                                    \
        }                                                                                                                       \
        lstm_forward_kernel<RES_, SAVE_><<<grid, kBlock, lds_bytes, stream>>>(row_ptr, col, n_dst, n_src, int(T), P, ldp, p_pad, \
                                                                              R, int(U), out_mean, ldo,                         \
                                                                              static_cast<float*>(saved), bad_flag);            \
    } while (0)
    if (res && saved != nullptr) TFGX_LSTM_FWD(true, true);
    else if (res) TFGX_LSTM_FWD(true, false);
    else if (saved != nullptr) TFGX_LSTM_FWD(false, true);
    else TFGX_LSTM_FWD(false, false);
#undef TFGX_LSTM_FWD
    TFGX_LAUNCH_CHECK("lstm_forward_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_lstm_aggregate_backward_f32(const int32_t* row_ptr, int64_t n_dst, int64_t T, int64_t U, const float* R,
                                                const float* d_mean, int64_t ldd, const void* saved, size_t saved_bytes,
                                                float* d_gates, float* h_prev, float* d_pad_partial, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_common(__func__, n_dst, T, U)) return rc;
    if (ldd < U) {
        set_error("%s: ldd is smaller than U (%lld < %lld)", __func__, (long long)ldd, (long long)U);
        return TFGX_ERR_INVALID_ARG;
    }
    if (n_dst == 0 || T == 0 || U == 0) return TFGX_OK;
    if (n_dst * T > kInt32Max) {
        set_error("%s: n_dst * T must fit int32 (rows of d_gates), got %lld", __func__, (long long)(n_dst * T));
        return TFGX_ERR_INVALID_ARG;
    }
    const void* ptrs[] = {row_ptr, R, d_mean, saved, d_gates, h_prev, d_pad_partial};
    const char* names[] = {"row_ptr", "R", "d_mean", "saved", "d_gates", "h_prev", "d_pad_partial"};
    for (int i = 0; i < 7; ++i)
        if (ptrs[i] == nullptr) {
            set_error("%s: %s is null", __func__, names[i]);
            return TFGX_ERR_INVALID_ARG;
        }
    if (saved_bytes < tfgx_lstm_aggregate_saved_bytes(n_dst, T, U)) {
        set_error("%s: saved_bytes is too small (%zu < %zu)", __func__, saved_bytes, tfgx_lstm_aggregate_saved_bytes(n_dst, T, U));
        return TFGX_ERR_INVALID_ARG;
    }
    const bool res = tfgx_lstm_recurrent_kernel_resident(U, 1) != 0;
    const size_t lds_bytes = bwd_lds_bytes(U, res);
    const int grid = int(tfgx_lstm_aggregate_tiles(n_dst));
#define TFGX_LSTM_BWD(RES_)                                                                                                     \
    do {                                                                                                                        \
        static bool attr_set = false;                                                                                           \
        if (!attr_set) {                                                                                                        \
            TFGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_backward_kernel<RES_>),                       \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, int(kLdsLimit)));                    \
            attr_set = true;                                                                                                    \
        }                                                                                                                       \
        lstm_backward_kernel<RES_><<<grid, kBlock, lds_bytes, stream>>>(row_ptr, n_dst, int(T), int(U), R, d_mean, ldd,         \
                                                                        static_cast<const float*>(saved), d_gates, h_prev,      \
                                                                        d_pad_partial);                                         \
    } while (0)
    if (res) TFGX_LSTM_BWD(true);
    else TFGX_LSTM_BWD(false);
#undef TFGX_LSTM_BWD
    TFGX_LAUNCH_CHECK("lstm_backward_kernel");
    return TFGX_OK;
}
