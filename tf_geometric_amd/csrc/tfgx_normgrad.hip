// Backward of the GCN normalisation (include/tfgx_normgrad.h): d/d(raw edge weight) of tfgx_segment_weight_sum_f32 +
// tfgx_gcn_norm_edges_f32 (tfgx_norm.hip), given the gradients of the normalised weights and of the self-loop coefficients.
// Reference: tf_geometric/nn/conv/gcn.py:32-130, differentiated by TensorFlow op by op.
//
// Three launches in tfgx_norm.hip's layout — one group of 8 lanes per row, rows longer than kLongRow edges left to the WHOLE
// workgroup after its short rows — so a hub row or hub column is never an 8-lane latency chain:
//   row pass   over the forward CSR: A[v] (BOTH) or D[v] (LEFT) per row, and the per-edge product t_e written in CSR order
//   col pass   over the transposed plan's row_ptr: B[v] = sum of t[t2d[j]] (ONE 4-byte random gather per edge), finished to D / D_c
//   edge pass  dw_e from G_e, the two degree factors and the node terms
// Every sum has a fixed order (lane-strided partials, a fixed shuffle tree, waves in order): no atomics on floats, bit-identical
// from run to run.  Long rows keep four independent gather chains per lane, as the forward does.
#include "tfgx_common.h"
#include "../../include/tfgx_normgrad.h"

namespace tfgx {
namespace {

constexpr int NG = 8;                      // lanes per row
constexpr int kLongRow = 2048;             // edges: longer rows are walked by the whole workgroup
constexpr int kRowsPerBlock = kBlock / NG;
// Grid cap: a PRIME number of workgroups.  A workgroup takes the 32-row tiles blockIdx, blockIdx + grid, ...; with a power-of-two
// grid the tiles of one workgroup start at multiples of 2^18, and the hubs of an R-MAT graph sit exactly at ids with few one-bits
// (0, 2^18, 2^19, 2^18 + 2^19, ...): one workgroup then walked 2.5 % of all edges of the products-sized R-MAT graph by itself.
constexpr int kGridCap = 8191;

__device__ __forceinline__ float group_sum(float v)
{
#pragma unroll
    for (int o = NG / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, NG);
    return v;
}

// sum over the workgroup, the same value in every thread: fixed tree inside the wave, waves in order
__device__ __forceinline__ float block_sum(float v, float* part)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.0f;
#pragma unroll
    for (int q = 0; q < kBlock / 64; ++q) t += part[q];
    __syncthreads();
    return t;
}

// the forward's factor: tf.pow(deg, -1/2 | -1) with inf / nan -> 0 (tfgx_norm.hip inv_pow)
__device__ __forceinline__ float inv_pow(float d, bool half)
{
    const float v = half ? (1.0f / sqrtf(d)) : (1.0f / d);
    return (isinf(v) || isnan(v)) ? 0.0f : v;
}

// its derivative: -1/2 d^-3/2 = -1/2 p^3, -d^-2 = -q^2; zero where the forward zeroed the factor, zero where not finite
__device__ __forceinline__ float inv_pow_grad(float d, bool half)
{
    const float f = inv_pow(d, half);
    const float v = half ? (-0.5f * f * f * f) : (-(f * f));
    return (isinf(v) || isnan(v)) ? 0.0f : v;
}

struct NormGradArgs {
    const int32_t* row_ptr;
    const int32_t* col;
    const float* w;
    int64_t n_rows, n_cols;
    const int32_t* t_row_ptr;
    const int32_t* t2d;
    const float* row_deg;
    const float* col_deg;     // NULL: the row degrees serve both sides
    float fill;
    int self_both;            // BOTH: add_self_loop && renorm && S
    int self_lr;              // LEFT / RIGHT: add_self_loop && S
    const float* G;
    const float* S;
    float* A;
    float* B;
    float* t;
    float* dw;
};

// The row-loop skeleton the three passes share.  `walk(r, first, step)` returns this lane's partial of row r over positions
// first, first + step, ...; `finish(r, total)` is called by one lane with the row's sum.  SUM = false: nothing is reduced.
template <bool SUM, class Walk, class Finish>
__device__ __forceinline__ void for_rows(const int32_t* __restrict__ row_ptr, int64_t n, Walk walk, Finish finish)
{
    __shared__ int long_rows[kRowsPerBlock];
    __shared__ int n_long;
    __shared__ float part[kBlock / 64];
    const int lane = threadIdx.x % NG, grp = threadIdx.x / NG;
    for (int64_t base = int64_t(blockIdx.x) * kRowsPerBlock; base < n; base += int64_t(gridDim.x) * kRowsPerBlock) {
        if (threadIdx.x == 0) n_long = 0;
        __syncthreads();
        const int64_t r = base + grp;
        if (r < n) {
            if (row_ptr[r + 1] - row_ptr[r] > kLongRow) {
                if (lane == 0) long_rows[atomicAdd(&n_long, 1)] = grp;    // (integer: arrival order changes no sum)
            } else {
                float acc = walk(r, lane, NG);
                if (SUM) {
                    acc = group_sum(acc);
                    if (lane == 0) finish(r, acc);
                }
            }
        }
        __syncthreads();
        const int nl = n_long;
        for (int k = 0; k < nl; ++k) {
            const int64_t rl = base + long_rows[k];
            float acc = walk(rl, int(threadIdx.x), kBlock);
            if (SUM) {
                acc = block_sum(acc, part);
                if (threadIdx.x == 0) finish(rl, acc);
            }
        }
        __syncthreads();
    }
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void normgrad_row_kernel(const NormGradArgs a)
{
    const float* __restrict__ G = a.G;
    const float* __restrict__ w = a.w;
    const int32_t* __restrict__ col = a.col;
    const float* __restrict__ cdeg = a.col_deg ? a.col_deg : a.row_deg;
    float* __restrict__ t = a.t;
    auto walk = [&](int64_t r, int first, int step) -> float {
        const int s = a.row_ptr[r], e = a.row_ptr[r + 1];
        if (MODE == TFGX_NORM_BOTH) {
            const float pr = inv_pow(a.row_deg[r], true);
            float acc4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            int i = s + first;
            // four independent col -> degree chains per lane (the forward's reason: a long row is bound by that gather's latency)
            for (; i + 3 * step < e; i += 4 * step) {
                int c4[4];
                float gw4[4], d4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { c4[u] = col[i + u * step]; gw4[u] = G[i + u * step] * w[i + u * step]; }
#pragma unroll
                for (int u = 0; u < 4; ++u) d4[u] = cdeg[c4[u]];
#pragma unroll
                for (int u = 0; u < 4; ++u) { t[i + u * step] = gw4[u] * pr; acc4[u] += gw4[u] * inv_pow(d4[u], true); }
            }
            float acc = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
            for (; i < e; i += step) {
                const float gw = G[i] * w[i];
                t[i] = gw * pr;
                acc += gw * inv_pow(cdeg[col[i]], true);
            }
            return acc;
        } else if (MODE == TFGX_NORM_LEFT) {
            float acc = 0.0f;
            for (int i = s + first; i < e; i += step) acc += G[i] * w[i];
            return acc;
        } else {
            for (int i = s + first; i < e; i += step) t[i] = G[i] * w[i];
            return 0.0f;
        }
    };
    auto finish = [&](int64_t r, float acc) {
        if (MODE == TFGX_NORM_BOTH) {
            if (a.self_both) acc += a.S[r] * a.fill * inv_pow(cdeg[r], true);
            a.A[r] = a.col_deg ? acc * inv_pow_grad(a.row_deg[r], true) : acc;     // D_r, or A for the col pass to finish
        } else {
            if (a.self_lr) acc += a.S[r] * a.fill;
            a.A[r] = acc * inv_pow_grad(a.row_deg[r], false);
        }
    };
    for_rows<MODE != TFGX_NORM_RIGHT>(a.row_ptr, a.n_rows, walk, finish);
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void normgrad_col_kernel(const NormGradArgs a)
{
    const float* __restrict__ t = a.t;
    const int32_t* __restrict__ t2d = a.t2d;
    auto walk = [&](int64_t v, int first, int step) -> float {
        const int s = a.t_row_ptr[v], e = a.t_row_ptr[v + 1];
        float acc4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int j = s + first;
        for (; j + 3 * step < e; j += 4 * step) {
            int p4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) p4[u] = t2d[j + u * step];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc4[u] += t[p4[u]];
        }
        float acc = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
        for (; j < e; j += step) acc += t[t2d[j]];
        return acc;
    };
    auto finish = [&](int64_t v, float acc) {
        if (MODE == TFGX_NORM_BOTH) {
            if (a.self_both) acc += a.S[v] * a.fill * inv_pow(a.row_deg[v], true);
            a.B[v] = a.col_deg ? acc * inv_pow_grad(a.col_deg[v], true)            // D_c
                               : (a.A[v] + acc) * inv_pow_grad(a.row_deg[v], true);   // D (square: v is a row too)
        } else {  // RIGHT (n_cols <= n_rows: row_deg[v] exists)
            if (a.self_lr) acc += a.S[v] * a.fill;
            a.B[v] = acc * inv_pow_grad(a.row_deg[v], false);
        }
    };
    for_rows<true>(a.t_row_ptr, a.n_cols, walk, finish);
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void normgrad_edge_kernel(const NormGradArgs a)
{
    const float* __restrict__ G = a.G;
    const int32_t* __restrict__ col = a.col;
    float* __restrict__ dw = a.dw;
    // every edge's value is independent: `first` / `step` only say which lanes walk the row
    auto walk = [&](int64_t r, int first, int step) -> float {
        const int s = a.row_ptr[r], e = a.row_ptr[r + 1];
        if (MODE == TFGX_NORM_BOTH) {
            const float pr = inv_pow(a.row_deg[r], true);
            if (a.col_deg) {
                const float dr = a.A[r];
                int i = s + first;
                for (; i + 3 * step < e; i += 4 * step) {
                    int c4[4];
                    float g4[4], d4[4], b4[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { c4[u] = col[i + u * step]; g4[u] = G[i + u * step]; }
#pragma unroll
                    for (int u = 0; u < 4; ++u) { d4[u] = a.col_deg[c4[u]]; b4[u] = a.B[c4[u]]; }
#pragma unroll
                    for (int u = 0; u < 4; ++u) dw[i + u * step] = g4[u] * pr * inv_pow(d4[u], true) + dr + b4[u];
                }
                for (; i < e; i += step) {
                    const int c = col[i];
                    dw[i] = G[i] * pr * inv_pow(a.col_deg[c], true) + dr + a.B[c];
                }
            } else {
                const float dr = a.B[r];
                int i = s + first;
                for (; i + 3 * step < e; i += 4 * step) {
                    int c4[4];
                    float g4[4], d4[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { c4[u] = col[i + u * step]; g4[u] = G[i + u * step]; }
#pragma unroll
                    for (int u = 0; u < 4; ++u) d4[u] = a.row_deg[c4[u]];
#pragma unroll
                    for (int u = 0; u < 4; ++u) dw[i + u * step] = g4[u] * pr * inv_pow(d4[u], true) + dr;
                }
                for (; i < e; i += step) dw[i] = G[i] * pr * inv_pow(a.row_deg[col[i]], true) + dr;
            }
        } else if (MODE == TFGX_NORM_LEFT) {
            const float qr = inv_pow(a.row_deg[r], false), dr = a.A[r];
            for (int i = s + first; i < e; i += step) dw[i] = G[i] * qr + dr;
        } else {  // RIGHT: the row degree of the COLUMN's node scales the edge; the degree term returns along the row
            const float dr = r < a.n_cols ? a.B[r] : 0.0f;
            for (int i = s + first; i < e; i += step) dw[i] = G[i] * inv_pow(a.row_deg[col[i]], false) + dr;
        }
        return 0.0f;
    };
    for_rows<false>(a.row_ptr, a.n_rows, walk, [](int64_t, float) {});
}

template <int MODE>
int launch_passes(const NormGradArgs& a, int passes, hipStream_t stream)
{
    const int grid_r = grid_for(a.n_rows, kRowsPerBlock, kGridCap);
    if (passes & TFGX_NORMGRAD_ROW_PASS) {
        normgrad_row_kernel<MODE><<<grid_r, kBlock, 0, stream>>>(a);
        TFGX_LAUNCH_CHECK("normgrad_row_kernel");
    }
    if constexpr (MODE != TFGX_NORM_LEFT) {
        if ((passes & TFGX_NORMGRAD_COL_PASS) && a.n_cols > 0) {
            normgrad_col_kernel<MODE><<<grid_for(a.n_cols, kRowsPerBlock, kGridCap), kBlock, 0, stream>>>(a);
            TFGX_LAUNCH_CHECK("normgrad_col_kernel");
        }
    }
    if (passes & TFGX_NORMGRAD_EDGE_PASS) {
        normgrad_edge_kernel<MODE><<<grid_r, kBlock, 0, stream>>>(a);
        TFGX_LAUNCH_CHECK("normgrad_edge_kernel");
    }
    return TFGX_OK;
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_normgrad_version(void) { return TFGX_NORMGRAD_ABI_VERSION; }

extern "C" int tfgx_gcn_norm_backward_f32(const int32_t* row_ptr, const int32_t* col, const float* w, int64_t n_rows,
                                          int64_t n_cols, const int32_t* t_row_ptr, const int32_t* t2d, const float* row_deg,
                                          const float* col_deg, int32_t norm_mode, float fill, int32_t add_self_loop,
                                          int32_t renorm, const float* G, const float* S, float* A, float* B, float* t, float* dw,
                                          int32_t passes, tfgx_stream_t stream)
{
    TFGX_RANGE();
    TFGX_REQUIRE(n_rows >= 0 && n_cols >= 0, "negative size");
    TFGX_REQUIRE(norm_mode >= TFGX_NORM_BOTH && norm_mode <= TFGX_NORM_RIGHT, "bad norm mode");
    TFGX_REQUIRE(passes > 0 && passes <= TFGX_NORMGRAD_ALL, "passes must be a non-empty subset of TFGX_NORMGRAD_ALL");
    TFGX_REQUIRE(w != nullptr, "w is null: an unweighted edge list has no weights to differentiate");
    TFGX_REQUIRE(!add_self_loop || n_rows == n_cols, "add_self_loop needs n_rows == n_cols");
    TFGX_REQUIRE(norm_mode != TFGX_NORM_BOTH || col_deg != nullptr || n_rows == n_cols,
                 "norm BOTH without col_deg (the symmetric form) needs n_rows == n_cols");
    TFGX_REQUIRE(norm_mode != TFGX_NORM_RIGHT || n_cols <= n_rows, "norm RIGHT needs n_cols <= n_rows");
    if (n_rows == 0) return TFGX_OK;
    TFGX_REQUIRE(row_ptr && col && row_deg && G && dw, "null pointer (row_ptr, col, row_deg, G, dw)");
    TFGX_REQUIRE(norm_mode == TFGX_NORM_RIGHT || A, "null pointer (A)");
    TFGX_REQUIRE(norm_mode == TFGX_NORM_LEFT || (t_row_ptr && t2d && B && t), "null pointer (t_row_ptr, t2d, B, t)");
    NormGradArgs a;
    a.row_ptr = row_ptr; a.col = col; a.w = w; a.n_rows = n_rows; a.n_cols = n_cols; a.t_row_ptr = t_row_ptr; a.t2d = t2d;
    a.row_deg = row_deg; a.col_deg = norm_mode == TFGX_NORM_BOTH ? col_deg : nullptr; a.fill = fill;
    a.self_both = (add_self_loop && renorm && S) ? 1 : 0;
    a.self_lr = (add_self_loop && S) ? 1 : 0;
    a.G = G; a.S = S; a.A = A; a.B = B; a.t = t; a.dw = dw;
    hipStream_t st = as_stream(stream);
    if (norm_mode == TFGX_NORM_BOTH) return launch_passes<TFGX_NORM_BOTH>(a, passes, st);
    if (norm_mode == TFGX_NORM_LEFT) return launch_passes<TFGX_NORM_LEFT>(a, passes, st);
    return launch_passes<TFGX_NORM_RIGHT>(a, passes, st);
}
