// Gather - scale - segment reduce over a 16-BIT feature table (bf16 / fp16 storage, fp32 arithmetic): include/tfgx_h16.h.
//
// The fp32 kernel (tfgx_reduce.hip) runs at the part's random-line ceiling: what a gathered row costs is the number of
// 128-byte lines it touches.  Stored in 16 bits a row touches half of them.  Nothing else changes: the mapping (a group of G
// lanes owns a destination row and broadcasts (col, w) inside the group), the row-header pipeline across rows, the masked
// partial batch and — the contract — the arithmetic.  Every element is widened in registers (bf16: a 16-bit shift, fp16:
// v_cvt_f32_f16, both exact) and then goes through exactly the expressions of seg_reduce_kernel, one in-order fp32 chain per
// output element in CSR edge order: fmaf(w, x, acc) / acc + x / fmaxf(acc, x * w), then accumulate, self_coef, the MEAN
// divisor, add_x, bias, activation.  A launch over a 16-bit table therefore returns, bit for bit, what
// tfgx_segment_reduce_f32 returns for that table widened to fp32 (tests/test_gpu_h16.py holds it to torch.equal), hub rows
// included: the chunk partials go through the same fp32 scratch and are folded in chunk order by the same finalize logic.
//
// Layout: rows are 16-byte aligned (ldx % 8 == 0, 16-byte aligned base), so every lane gathers ONE 16-byte vector of 8
// elements per chunk whatever F is: the columns in [F, roundup8(F)) are inside the row stride, they are read and discarded.
// This file copies what it needs from tfgx_reduce.hip on purpose: that file's code generation must not move.
#include "tfgx_common.h"
#include "tfgx_widen_h16.h"
#include "../../include/tfgx_h16.h"
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace tfgx {
namespace {

template <int G>
__device__ __forceinline__ int bcast_i(int v, int j)
{
    if constexpr (G == 64) return __builtin_amdgcn_readlane(v, j);
    else return __shfl(v, j, G);
}
template <int G>
__device__ __forceinline__ float bcast_f(float v, int j)
{
    if constexpr (G == 64) return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
    else return __shfl(v, j, G);
}

struct HArgs {
    const int32_t* row_begin;
    const int32_t* row_end;
    int64_t rp_stride;
    const int32_t* col;
    const float* w;
    int64_t n_dst;
    const uint16_t* x;        // [n_src, ldx] 16-bit elements
    int64_t ldx;
    int32_t F;
    void* out;                // [n_dst, ldo] floats, or 16-bit elements of out_dt
    int64_t ldo;
    int32_t out_dt;           // TFGX_DT_F32 / TFGX_DT_BF16 / TFGX_DT_F16
    int32_t f32_vec;          // every fp32 row the epilogue touches (out, add_x, bias) is 16-byte aligned: float4 accesses
    int32_t h16_vec;          // a 16-bit out has 16-byte aligned rows: one 16-byte store per full vector
    int32_t op, act, accumulate;
    const float* self_coef;
    const float* bias;
    const float* add_x;
    int64_t ld_add;
    const int32_t* mean_count;
    int32_t hub_threshold;    // > 0: rows with more edges than this are left to the hub path
    const int32_t* row_order;
    int32_t wide_blocks;
};

// ---- 16-bit <-> fp32 in registers (widen1 / widen8: tfgx_widen_h16.h).  Widening is exact; narrowing is round-to-nearest-even,
// NaN stays NaN.
__device__ __forceinline__ float widen_rt(uint32_t bits16, int dt)
{
    return dt == TFGX_DT_BF16 ? widen1<TFGX_DT_BF16>(bits16) : widen1<TFGX_DT_F16>(bits16);
}

__device__ __forceinline__ uint32_t narrow_rt(float f, int dt)
{
    if (dt == TFGX_DT_BF16) {
        const uint32_t u = __float_as_uint(f);
        if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;      // NaN: keep it one (quiet bit set)
        return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;                        // round to nearest, ties to even
    }
    return uint32_t(__builtin_bit_cast(unsigned short, static_cast<_Float16>(f)));   // v_cvt_f16_f32: RNE, overflow -> inf
}

// 8 consecutive floats of a row, the first `nv` of them inside the row (the rest read as 0 and are never stored)
__device__ __forceinline__ void load8_f32(const float* p, bool vec, int nv, float (&v)[kVec])
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (vec && nv >= 4 * h + 4) {
            const float4 t = *reinterpret_cast<const float4*>(p + 4 * h);
            v[4 * h] = t.x; v[4 * h + 1] = t.y; v[4 * h + 2] = t.z; v[4 * h + 3] = t.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[4 * h + i] = (4 * h + i < nv) ? p[4 * h + i] : 0.0f;
        }
    }
}

__device__ __forceinline__ void store8_h16(uint16_t* p, bool vec, int nv, int dt, const float (&v)[kVec])
{
    uint32_t b[kVec];
#pragma unroll
    for (int i = 0; i < kVec; ++i) b[i] = narrow_rt(v[i], dt);
    if (vec && nv == kVec) {
        *reinterpret_cast<uint4*>(p) = make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16));
    } else {
#pragma unroll
        for (int i = 0; i < kVec; ++i)
            if (i < nv) p[i] = uint16_t(b[i]);
    }
}

#ifndef TFGX_REDUCE_GRID_CAP_DEFAULT
#define TFGX_REDUCE_GRID_CAP_DEFAULT (1 << 20)
#endif

// One destination row [s, e) of the plan, reduced by a group of G lanes.
// U: edges per batch (0 = the default for the group shape: 8, 4 with two column chunks per lane).
template <int DT, int G, int CH, bool IS_MAX, bool WEIGHTED, int U>
__device__ __forceinline__ void seg_reduce_h16_row(const HArgs& a, int64_t r, int s, int e, int cj_next, float wj_next, int lane,
                                                   const int (&coff)[CH], const bool (&cvalid)[CH], float init)
{
    constexpr int UNROLL_W = U > 0 ? U : (CH >= 2 ? 4 : 8);
    constexpr int UNROLL = UNROLL_W < G ? UNROLL_W : G;
    float acc[CH][kVec];
#pragma unroll
    for (int k = 0; k < CH; ++k)
#pragma unroll
        for (int v = 0; v < kVec; ++v) acc[k][v] = init;

    // (col, w) of the NEXT batch are loaded while the current batch's rows are in flight
    for (int base = s; base < e; base += G) {
        const int cj = cj_next;
        const float wj = wj_next;
        const int nxt = base + G + lane;
        if (nxt < e) {
            cj_next = a.col[nxt];
            if constexpr (WEIGHTED) wj_next = a.w[nxt];
        }
        const int cnt = min(G, e - base);
        // UNROLL independent 16-byte loads in flight per lane before the first FMA.  The last, partial batch is ONE batch too
        // (masked = true): the loads of the missing slots repeat the last edge's (clamped index: the same lines, an L1 hit),
        // the arithmetic of a missing slot is dropped by a SELECT — a branch there lets the compiler sink the slot's load
        // into it and wait for it alone.
        auto batch = [&](int j, auto masked) {
            constexpr bool MASKED = decltype(masked)::value;
            uint4 raw[UNROLL][CH];
            float ww[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int idx = MASKED ? min(j + u, cnt - 1) : j + u;
                const int c = bcast_i<G>(cj, idx);
                if constexpr (WEIGHTED) ww[u] = bcast_f<G>(wj, idx);
#pragma unroll
                for (int k = 0; k < CH; ++k) raw[u][k] = *reinterpret_cast<const uint4*>(a.x + int64_t(c) * a.ldx + coff[k]);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const bool live = !MASKED || j + u < cnt;
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    float xv[kVec];
                    widen8<DT>(raw[u][k], xv);
#pragma unroll
                    for (int v = 0; v < kVec; ++v) {
                        if constexpr (IS_MAX) {
                            const float m = WEIGHTED ? xv[v] * ww[u] : xv[v];
                            const float t = fmaxf(acc[k][v], m);
                            acc[k][v] = live ? t : acc[k][v];
                        } else {
                            const float t = WEIGHTED ? fmaf(ww[u], xv[v], acc[k][v]) : acc[k][v] + xv[v];
                            acc[k][v] = live ? t : acc[k][v];
                        }
                    }
                }
            }
        };
        int j = 0;
        for (; j + UNROLL <= cnt; j += UNROLL) batch(j, std::false_type{});
        if (j < cnt) batch(j, std::true_type{});
    }

    // ---- epilogue (per destination row): the fp32 kernel's, term by term
    const float sc = a.self_coef ? a.self_coef[r] : 0.0f;
    float divisor = 1.0f;
    if (a.op == TFGX_MEAN) {
        const int cnt = a.mean_count ? a.mean_count[r] : (e - s);
        divisor = float(cnt > 1 ? cnt : 1);
    }
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        if (!cvalid[k]) continue;
        const int nv = min(kVec, a.F - coff[k]);
        float res[kVec];
#pragma unroll
        for (int v = 0; v < kVec; ++v) res[v] = acc[k][v];
        if (a.accumulate) {          // fp32 outputs only (checked on the host)
            float prev[kVec];
            load8_f32(static_cast<const float*>(a.out) + r * a.ldo + coff[k], a.f32_vec != 0, nv, prev);
#pragma unroll
            for (int v = 0; v < kVec; ++v) res[v] = IS_MAX ? fmaxf(prev[v], res[v]) : prev[v] + res[v];
        }
        if (a.self_coef) {
            float xself[kVec];
            widen8<DT>(*reinterpret_cast<const uint4*>(a.x + r * a.ldx + coff[k]), xself);
#pragma unroll
            for (int v = 0; v < kVec; ++v) {
                if constexpr (IS_MAX) res[v] = fmaxf(res[v], sc * xself[v]);
                else res[v] = fmaf(sc, xself[v], res[v]);
            }
        }
        if (a.op == TFGX_MEAN) {
#pragma unroll
            for (int v = 0; v < kVec; ++v) res[v] = res[v] / divisor;
        }
        if (a.add_x) {
            float xa[kVec];
            load8_f32(a.add_x + r * a.ld_add + coff[k], a.f32_vec != 0, nv, xa);
#pragma unroll
            for (int v = 0; v < kVec; ++v) res[v] = xa[v] + res[v];
        }
        if (a.bias) {
            float b[kVec];
            load8_f32(a.bias + coff[k], a.f32_vec != 0, nv, b);
#pragma unroll
            for (int v = 0; v < kVec; ++v) res[v] += b[v];
        }
#pragma unroll
        for (int v = 0; v < kVec; ++v) res[v] = apply_act(res[v], a.act);
        if (a.out_dt == TFGX_DT_F32) store8_f32(static_cast<float*>(a.out) + r * a.ldo + coff[k], a.f32_vec != 0, nv, res);
        else store8_h16(static_cast<uint16_t*>(a.out) + r * a.ldo + coff[k], a.h16_vec != 0, nv, a.out_dt, res);
    }
}

template <int DT, int G, int CH, bool IS_MAX, bool WEIGHTED, int U>
__global__ __launch_bounds__(kBlock) void seg_reduce_h16_kernel(const HArgs a)
{
    constexpr int ROWS_PER_BLOCK = kBlock / G;
    constexpr int COLS_PER_PASS = G * kVec * CH;
    const int lane = threadIdx.x % G;
    const int grp = threadIdx.x / G;
    // column blocks on grid.y (wide rows, and rows wider than 64 lanes x CH chunks): see tfgx_reduce.hip
    const int colbase = blockIdx.y * COLS_PER_PASS;

    // column offsets of this lane; lanes past F read, branch-free and discarded, their OWN vector of pad columns while it is
    // inside the row stride (the [n_src, ldx] table is readable up to ldx in every row), else the row's first vector.  Going
    // back to column 0 costs: F = 100 on a 128-element stride ran its hub chunks 32 % slower than F = 128 on the same stride
    // with equal L2 request and miss counts, three pad lanes pulling the first line into the quad that reads the second.
    int coff[CH];
    bool cvalid[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        const int c = colbase + (k * G + lane) * kVec;
        cvalid[k] = c < a.F;
        coff[k] = (cvalid[k] || int64_t(c) + kVec <= a.ldx) ? c : 0;
    }
    const float init = IS_MAX ? -FLT_MAX : 0.0f;

    // the header chain of a row — row_ptr -> first (col, w) batch -> first gathered rows — is software-pipelined across the
    // rows a lane group walks: while row r is reduced, the first (col, w) batch of row r + stride and the (begin, end) pair
    // of row r + 2 * stride are already in flight
    const int64_t rstride = int64_t(gridDim.x) * ROWS_PER_BLOCK;
    int64_t r = int64_t(blockIdx.x) * ROWS_PER_BLOCK + grp;
    auto row_of = [&](int64_t i) -> int64_t { return a.row_order ? int64_t(a.row_order[i]) : i; };
    int s = 0, e = 0, s1 = 0, e1 = 0;
    if (r < a.n_dst) {
        const int64_t q = row_of(r);
        s = a.row_begin[q * a.rp_stride];
        e = a.row_end[q * a.rp_stride];
    }
    if (r + rstride < a.n_dst) {
        const int64_t q = row_of(r + rstride);
        s1 = a.row_begin[q * a.rp_stride];
        e1 = a.row_end[q * a.rp_stride];
    }
    int cj_first = 0;
    float wj_first = 0.0f;
    if (s + lane < e) {
        cj_first = a.col[s + lane];
        if constexpr (WEIGHTED) wj_first = a.w[s + lane];
    }
    for (; r < a.n_dst; r += rstride) {
        int s2 = 0, e2 = 0;                                       // header of the row after next
        if (r + 2 * rstride < a.n_dst) {
            const int64_t q = row_of(r + 2 * rstride);
            s2 = a.row_begin[q * a.rp_stride];
            e2 = a.row_end[q * a.rp_stride];
        }
        int cj_first1 = 0;                                        // first (col, w) batch of the next row
        float wj_first1 = 0.0f;
        if (s1 + lane < e1) {
            cj_first1 = a.col[s1 + lane];
            if constexpr (WEIGHTED) wj_first1 = a.w[s1 + lane];
        }
        const int s_cur = G == 64 ? __builtin_amdgcn_readfirstlane(s) : s;
        const int e_cur = G == 64 ? __builtin_amdgcn_readfirstlane(e) : e;
        const int cj_next = cj_first;
        const float wj_next = wj_first;
        s = s1; e = e1; s1 = s2; e1 = e2; cj_first = cj_first1; wj_first = wj_first1;      // rotate the pipeline
        if (a.hub_threshold > 0 && e_cur - s_cur > a.hub_threshold) continue;   // handled by the chunked hub path
        seg_reduce_h16_row<DT, G, CH, IS_MAX, WEIGHTED, U>(a, row_of(r), s_cur, e_cur, cj_next, wj_next, lane, coff, cvalid, init);
    }
}

inline int reduce_grid_cap()
{
    static int cap = 0;
    if (cap == 0) {
        const char* e = getenv("TFGX_REDUCE_GRID_CAP");
        cap = (e != nullptr && atoi(e) > 0) ? atoi(e) : TFGX_REDUCE_GRID_CAP_DEFAULT;
    }
    return cap;
}

// Group shape of a launch: lanes per row G, column chunks per lane CH, column blocks on grid.y NY, edges per batch U
// (0 = default) — the ONE place it is decided (launch_dt dispatches on it, tfgx_segment_reduce_h16_describe reports it).
struct GroupShape { int G, CH, NY, U; };

inline GroupShape group_shape(const HArgs& a)
{
    const int lanes = (a.F + kVec - 1) / kVec;
    // wide rows made of whole 128-byte lines (F >= 256 elements = 512 bytes, F % 64 == 0, line-aligned table): column blocks
    // of 128 elements (256 bytes, two lines per gathered piece) on grid.y, 16 pieces in flight per lane — the shape the fp32
    // kernel runs its wide rows at.  ONLY on request (wide_blocks > 0): the same-box A/B of tools/bench_half_features.py is
    // recorded in docs/DESIGN_LEDGER.md.
    if (a.F >= 256 && a.F % 64 == 0 && a.ldx % 64 == 0 && aligned_to(a.x, 128) && a.wide_blocks > 0)
        return GroupShape{16, 1, (lanes + 15) / 16, 16};
    if (lanes <= 4) return GroupShape{4, 1, 1, 0};
    if (lanes <= 8) return GroupShape{8, 1, 1, 0};
    if (lanes <= 16) return GroupShape{16, 1, 1, 0};
    if (lanes <= 32) return GroupShape{32, 1, 1, 0};
    if (lanes <= 64) return GroupShape{64, 1, 1, 0};
    const int per = 64 * 2;      // wider rows: column blocks of 64 lanes x 2 chunks on grid.y (col / w re-read per block)
    return GroupShape{64, 2, (lanes + per - 1) / per, 0};
}

template <int DT, int G, int CH, int U>
int launch_cfg(const HArgs& a, bool is_max, bool weighted, int ny, hipStream_t stream)
{
    constexpr int ROWS_PER_BLOCK = kBlock / G;
    dim3 grid(grid_for(a.n_dst, ROWS_PER_BLOCK, CH >= 2 ? (reduce_grid_cap() < 4096 ? reduce_grid_cap() : 4096) : reduce_grid_cap()), ny, 1);
    dim3 block(kBlock, 1, 1);
    if (is_max) {
        if (weighted) seg_reduce_h16_kernel<DT, G, CH, true, true, U><<<grid, block, 0, stream>>>(a);
        else seg_reduce_h16_kernel<DT, G, CH, true, false, U><<<grid, block, 0, stream>>>(a);
    } else {
        if (weighted) seg_reduce_h16_kernel<DT, G, CH, false, true, U><<<grid, block, 0, stream>>>(a);
        else seg_reduce_h16_kernel<DT, G, CH, false, false, U><<<grid, block, 0, stream>>>(a);
    }
    TFGX_LAUNCH_CHECK("seg_reduce_h16_kernel");
    return TFGX_OK;
}

template <int DT>
int launch_dt(const HArgs& a, bool is_max, bool weighted, hipStream_t stream)
{
    const GroupShape g = group_shape(a);
    if (g.U == 16) return launch_cfg<DT, 16, 1, 16>(a, is_max, weighted, g.NY, stream);
    if (g.CH == 2) return launch_cfg<DT, 64, 2, 0>(a, is_max, weighted, g.NY, stream);
    switch (g.G) {
        case 4: return launch_cfg<DT, 4, 1, 0>(a, is_max, weighted, 1, stream);
        case 8: return launch_cfg<DT, 8, 1, 0>(a, is_max, weighted, 1, stream);
        case 16: return launch_cfg<DT, 16, 1, 0>(a, is_max, weighted, 1, stream);
        case 32: return launch_cfg<DT, 32, 1, 0>(a, is_max, weighted, 1, stream);
        default: return launch_cfg<DT, 64, 1, 0>(a, is_max, weighted, 1, stream);
    }
}

int launch_any(const HArgs& a, int x_dt, bool is_max, bool weighted, hipStream_t stream)
{
    if (x_dt == TFGX_DT_BF16) return launch_dt<TFGX_DT_BF16>(a, is_max, weighted, stream);
    return launch_dt<TFGX_DT_F16>(a, is_max, weighted, stream);
}

// Hub rows: the chunk partials (fp32 scratch, written by a second launch of the kernel above over the chunk list) folded IN
// CHUNK ORDER, then the epilogue — hub_finalize_kernel of tfgx_reduce.hip with the row's own features read from the 16-bit
// table and the result stored in the output's type.
struct HubArgs {
    const int32_t* hub_rows;
    const int32_t* hub_chunk_ptr;
    const float* scratch;
    int64_t n_hub;
    int32_t x_dt;
    HArgs k;
};

__global__ __launch_bounds__(kBlock) void hub_finalize_h16_kernel(const HubArgs h)
{
    const HArgs& a = h.k;
    const bool is_max = a.op == TFGX_MAX;
    int64_t t = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    const int64_t total = h.n_hub * a.F;
    for (; t < total; t += stride) {
        const int64_t i = t / a.F;
        const int j = int(t - i * a.F);
        const int64_t r = h.hub_rows[i];
        float res = is_max ? -FLT_MAX : 0.0f;
        constexpr int HB = 16;
        int c = h.hub_chunk_ptr[i];
        const int c_end = h.hub_chunk_ptr[i + 1];
        const float* sp = h.scratch + int64_t(c) * a.F + j;
        for (; c + HB <= c_end; c += HB, sp += int64_t(HB) * a.F) {
            float v[HB];
#pragma unroll
            for (int u = 0; u < HB; ++u) v[u] = __builtin_nontemporal_load(sp + int64_t(u) * a.F);
#pragma unroll
            for (int u = 0; u < HB; ++u) res = is_max ? fmaxf(res, v[u]) : res + v[u];
        }
        for (; c < c_end; ++c, sp += a.F) {
            const float v = *sp;
            res = is_max ? fmaxf(res, v) : res + v;
        }
        float* op = static_cast<float*>(a.out) + r * a.ldo + j;
        if (a.accumulate) res = is_max ? fmaxf(*op, res) : *op + res;
        if (a.self_coef) {
            const float xv = widen_rt(a.x[r * a.ldx + j], h.x_dt);
            res = is_max ? fmaxf(res, a.self_coef[r] * xv) : fmaf(a.self_coef[r], xv, res);
        }
        if (a.op == TFGX_MEAN) {
            const int cnt = a.mean_count ? a.mean_count[r]
                                         : (a.row_end[r * a.rp_stride] - a.row_begin[r * a.rp_stride]);
            res = res / float(cnt > 1 ? cnt : 1);
        }
        if (a.add_x) res = a.add_x[r * a.ld_add + j] + res;
        if (a.bias) res += a.bias[j];
        res = apply_act(res, a.act);
        if (a.out_dt == TFGX_DT_F32) *op = res;
        else static_cast<uint16_t*>(a.out)[r * a.ldo + j] = uint16_t(narrow_rt(res, a.out_dt));
    }
}

// ---- converters: [n, F] rows, independent leading dimensions, one thread per (row, 8 columns), grid-stride.
__global__ __launch_bounds__(kBlock) void rows_f32_to_h16_kernel(const float* __restrict__ src, int64_t ld_src, int64_t n, int F,
                                                                 uint16_t* __restrict__ dst, int64_t ld_dst, int dt, int src_vec,
                                                                 int dst_vec)
{
    const int per_row = (F + kVec - 1) / kVec;
    const int64_t total = n * per_row;
    for (int64_t t = blockIdx.x * int64_t(kBlock) + threadIdx.x; t < total; t += int64_t(gridDim.x) * kBlock) {
        const int64_t i = t / per_row;
        const int j = int(t - i * per_row) * kVec;
        const int nv = min(kVec, F - j);
        float v[kVec];
        load8_f32(src + i * ld_src + j, src_vec != 0, nv, v);
        store8_h16(dst + i * ld_dst + j, dst_vec != 0, nv, dt, v);      // columns in [F, ld_dst) are never written
    }
}

__global__ __launch_bounds__(kBlock) void rows_h16_to_f32_kernel(const uint16_t* __restrict__ src, int64_t ld_src, int dt, int64_t n,
                                                                 int F, float* __restrict__ dst, int64_t ld_dst, int src_vec,
                                                                 int dst_vec)
{
    const int per_row = (F + kVec - 1) / kVec;
    const int64_t total = n * per_row;
    for (int64_t t = blockIdx.x * int64_t(kBlock) + threadIdx.x; t < total; t += int64_t(gridDim.x) * kBlock) {
        const int64_t i = t / per_row;
        const int j = int(t - i * per_row) * kVec;
        const int nv = min(kVec, F - j);
        const uint16_t* sp = src + i * ld_src + j;
        float v[kVec];
        if (src_vec && nv == kVec) {
            const uint4 raw = *reinterpret_cast<const uint4*>(sp);
            if (dt == TFGX_DT_BF16) widen8<TFGX_DT_BF16>(raw, v);
            else widen8<TFGX_DT_F16>(raw, v);
        } else {
#pragma unroll
            for (int k = 0; k < kVec; ++k) v[k] = k < nv ? widen_rt(sp[k], dt) : 0.0f;
        }
        store8_f32(dst + i * ld_dst + j, dst_vec != 0, nv, v);
    }
}

// The host checks both entry points share; fills the kernel arguments.
int check_and_fill(const char* fn, const tfgx_reduce_args* p, int32_t x_dtype, int32_t out_dtype, HArgs* a)
{
#define H16_REQUIRE(cond, msg)                       \
    do {                                             \
        if (!(cond)) {                               \
            set_error("%s: %s", fn, msg);            \
            return TFGX_ERR_INVALID_ARG;             \
        }                                            \
    } while (0)
    H16_REQUIRE(p != nullptr, "args is null");
    H16_REQUIRE(is_h16(x_dtype), "bad x_dtype (TFGX_DT_BF16 or TFGX_DT_F16)");
    H16_REQUIRE(out_dtype == TFGX_DT_F32 || is_h16(out_dtype), "bad out_dtype (TFGX_DT_F32, TFGX_DT_BF16 or TFGX_DT_F16)");
    // F: the widest shapes put up to ceil(F / 128) column blocks on grid.y, which holds 65535
    H16_REQUIRE(p->n_dst >= 0 && p->F >= 1 && p->F <= int64_t(65535) * 128, "bad n_dst / F (F must be in [1, 65535 * 128])");
    H16_REQUIRE(p->op == TFGX_SUM || p->op == TFGX_MEAN || p->op == TFGX_MAX, "bad op");
    H16_REQUIRE(p->act == TFGX_ACT_NONE || p->act == TFGX_ACT_RELU, "bad act");
    H16_REQUIRE(p->x_tail == nullptr, "x_tail: the split-row layout is not supported on a 16-bit table");
    H16_REQUIRE(p->edge_tail == nullptr, "edge_tail: the split-row layout is not supported on a 16-bit table");
    H16_REQUIRE(p->verify == 0, "verify: the verified layout is not supported on a 16-bit table");
    H16_REQUIRE(p->track == nullptr, "track: not supported on a 16-bit table (max aggregation is inference-only)");
    H16_REQUIRE(p->ldx % kVec == 0, "ldx: rows of a 16-bit table must be 16-byte aligned (ldx % 8 == 0)");
    H16_REQUIRE(aligned_to(p->x, 16), "x: rows of a 16-bit table must be 16-byte aligned (misaligned base)");
    H16_REQUIRE(!(p->accumulate && out_dtype != TFGX_DT_F32), "accumulate: needs a float32 output");
    H16_REQUIRE(p->ldx >= p->F && p->ldo >= p->F, "leading dimension < F");
    H16_REQUIRE(p->rp_stride >= 1, "rp_stride < 1");
    H16_REQUIRE(!(p->add_x) || p->ld_add >= p->F, "ld_add < F");
    H16_REQUIRE(aligned_to(p->out, out_dtype == TFGX_DT_F32 ? 4 : 2), "out: misaligned");
#undef H16_REQUIRE
    a->row_begin = p->row_begin; a->row_end = p->row_end; a->rp_stride = p->rp_stride;
    a->col = p->col; a->w = p->w; a->n_dst = p->n_dst;
    a->x = static_cast<const uint16_t*>(static_cast<const void*>(p->x)); a->ldx = p->ldx; a->F = int32_t(p->F);
    a->out = p->out; a->ldo = p->ldo; a->out_dt = out_dtype;
    bool fv = true;
    if (out_dtype == TFGX_DT_F32) fv = fv && p->ldo % 4 == 0 && aligned_to(p->out, 16);
    if (p->add_x) fv = fv && p->ld_add % 4 == 0 && aligned_to(p->add_x, 16);
    if (p->bias) fv = fv && aligned_to(p->bias, 16);
    a->f32_vec = fv ? 1 : 0;
    a->h16_vec = (out_dtype != TFGX_DT_F32 && p->ldo % kVec == 0 && aligned_to(p->out, 16)) ? 1 : 0;
    a->op = p->op; a->act = p->act; a->accumulate = p->accumulate;
    a->self_coef = p->self_coef; a->bias = p->bias; a->add_x = p->add_x; a->ld_add = p->ld_add;
    a->mean_count = p->mean_count;
    a->hub_threshold = 0;
    a->row_order = p->row_order;
    a->wide_blocks = p->wide_blocks;
    return TFGX_OK;
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_h16_version(void) { return TFGX_H16_ABI_VERSION; }

// Average number of 128-byte lines a row of `row` bytes touches when rows start `stride` bytes apart (16-byte aligned rows).
static double h16_avg_lines(int64_t row, int64_t stride)
{
    int64_t g = stride % 128, b = 128;
    while (g != 0) { const int64_t t = b % g; b = g; g = t; }       // b = gcd(stride, 128)
    const int64_t period = 128 / b;
    int64_t lines = 0;
    for (int64_t i = 0; i < period; ++i) lines += ((i * stride) % 128 + row - 1) / 128 + 1;
    return double(lines) / double(period);
}

extern "C" int64_t tfgx_h16_friendly_ld(int64_t F)
{
    if (F <= 0) return kVec;
    const int64_t r8 = (F + 7) / 8 * 8;
    // plan.gather_friendly_ld at 2 bytes per element: the dense 16-byte aligned stride, the next multiple of 64 and of 128
    // bytes, the next power of two for narrow rows; fewest lines per row on average, ties to the smaller stride
    int64_t cands[4] = {r8, (F + 31) / 32 * 32, (F + 63) / 64 * 64, r8};
    if (F <= 64) {
        int64_t p = 8;
        while (p < F) p <<= 1;
        cands[3] = p;
    }
    int64_t best = 0;
    double best_lines = 0.0;
    for (int i = 0; i < 4; ++i) {
        const double l = h16_avg_lines(2 * r8, 2 * cands[i]);       // the kernel reads whole 16-byte vectors: roundup8(F) elements
        if (best == 0 || l < best_lines - 1e-9 || (l < best_lines + 1e-9 && cands[i] < best)) {
            best = cands[i];
            best_lines = l;
        }
    }
    // never a power-of-two row stride of 512 bytes or more (plan.pow2_row_stride): one more line between rows
    if (best >= 256 && (best & (best - 1)) == 0) best += 64;
    return best;
}

extern "C" int tfgx_segment_reduce_h16_describe(const tfgx_reduce_args* p, int32_t x_dtype, int32_t out_dtype, char* buf,
                                                size_t buf_bytes)
{
    TFGX_REQUIRE(buf != nullptr && buf_bytes > 0, "null buffer");
    buf[0] = '\0';
    HArgs a;
    const int rc = check_and_fill(__func__, p, x_dtype, out_dtype, &a);
    if (rc != TFGX_OK) return rc;
    const GroupShape g = group_shape(a);
    char name[128];
    const int len = snprintf(name, sizeof(name), "seg_reduce_h16_kernel<%d, %d, %d, %s, %s, %d>", int(x_dtype), g.G, g.CH,
                             p->op == TFGX_MAX ? "true" : "false", p->w ? "true" : "false", g.U);
    TFGX_REQUIRE(size_t(len) + 1 <= buf_bytes, "buffer too small");
    memcpy(buf, name, size_t(len) + 1);
    return TFGX_OK;
}

extern "C" int tfgx_segment_reduce_h16(const tfgx_reduce_args* p, int32_t x_dtype, int32_t out_dtype, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    HArgs a;
    int rc = check_and_fill(__func__, p, x_dtype, out_dtype, &a);
    if (rc != TFGX_OK) return rc;
    if (p->n_dst == 0) return TFGX_OK;
    TFGX_REQUIRE(p->row_begin && p->row_end && p->out && p->x, "null pointer");
    const bool use_hub = p->hub_threshold > 0 && p->n_hub_rows > 0;
    if (use_hub) {
        TFGX_REQUIRE(p->hub_rows && p->hub_chunk_ptr && p->hub_chunk_begin && p->hub_chunk_end && p->hub_scratch &&
                         p->n_hub_chunks > 0,
                     "hub rows given without chunk lists / scratch");
        a.hub_threshold = p->hub_threshold;
    }
    const bool is_max = p->op == TFGX_MAX;
    const bool weighted = p->w != nullptr;
    hipStream_t stream = as_stream(stream_);
    rc = launch_any(a, x_dtype, is_max, weighted, stream);
    if (rc != TFGX_OK || !use_hub) return rc;

    // hub path: (2) chunk partials -> fp32 scratch, (3) ordered fold + epilogue
    HArgs c = a;
    c.row_begin = p->hub_chunk_begin; c.row_end = p->hub_chunk_end; c.rp_stride = 1;
    c.n_dst = p->n_hub_chunks; c.out = p->hub_scratch; c.ldo = p->F; c.out_dt = TFGX_DT_F32;
    c.f32_vec = (p->F % 4 == 0 && aligned_to(p->hub_scratch, 16)) ? 1 : 0;
    c.h16_vec = 0;
    c.op = is_max ? TFGX_MAX : TFGX_SUM; c.act = TFGX_ACT_NONE; c.accumulate = 0;
    c.self_coef = nullptr; c.bias = nullptr; c.add_x = nullptr; c.mean_count = nullptr; c.hub_threshold = 0;
    c.row_order = nullptr;
    rc = launch_any(c, x_dtype, is_max, weighted, stream);
    if (rc != TFGX_OK) return rc;
    HubArgs h;
    h.hub_rows = p->hub_rows; h.hub_chunk_ptr = p->hub_chunk_ptr; h.scratch = p->hub_scratch;
    h.n_hub = p->n_hub_rows; h.x_dt = x_dtype; h.k = a;
    hub_finalize_h16_kernel<<<grid_for(p->n_hub_rows * p->F, kBlock), kBlock, 0, stream>>>(h);
    TFGX_LAUNCH_CHECK("hub_finalize_h16_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_rows_f32_to_h16(const float* src, int64_t ld_src, int64_t n, int64_t F, void* dst, int64_t ld_dst, int32_t dtype,
                                    tfgx_stream_t stream)
{
    TFGX_RANGE();
    TFGX_REQUIRE(n >= 0 && F >= 0 && F < (int64_t(1) << 30), "negative n / F");
    TFGX_REQUIRE(is_h16(dtype), "bad dtype (TFGX_DT_BF16 or TFGX_DT_F16)");
    if (n == 0 || F == 0) return TFGX_OK;
    TFGX_REQUIRE(src != nullptr && dst != nullptr, "null pointer");
    TFGX_REQUIRE(ld_src >= F && ld_dst >= F, "leading dimension < F");
    TFGX_REQUIRE(aligned_to(src, 4) && aligned_to(dst, 2), "misaligned pointer");
    const int sv = (ld_src % 4 == 0 && aligned_to(src, 16)) ? 1 : 0;
    const int dv = (ld_dst % kVec == 0 && aligned_to(dst, 16)) ? 1 : 0;
    rows_f32_to_h16_kernel<<<grid_for(n * ((F + kVec - 1) / kVec), kBlock), kBlock, 0, as_stream(stream)>>>(
        src, ld_src, n, int(F), static_cast<uint16_t*>(dst), ld_dst, int(dtype), sv, dv);
    TFGX_LAUNCH_CHECK("rows_f32_to_h16_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_rows_h16_to_f32(const void* src, int64_t ld_src, int32_t dtype, int64_t n, int64_t F, float* dst, int64_t ld_dst,
                                    tfgx_stream_t stream)
{
    TFGX_RANGE();
    TFGX_REQUIRE(n >= 0 && F >= 0 && F < (int64_t(1) << 30), "negative n / F");
    TFGX_REQUIRE(is_h16(dtype), "bad dtype (TFGX_DT_BF16 or TFGX_DT_F16)");
    if (n == 0 || F == 0) return TFGX_OK;
    TFGX_REQUIRE(src != nullptr && dst != nullptr, "null pointer");
    TFGX_REQUIRE(ld_src >= F && ld_dst >= F, "leading dimension < F");
    TFGX_REQUIRE(aligned_to(src, 2) && aligned_to(dst, 4), "misaligned pointer");
    const int sv = (ld_src % kVec == 0 && aligned_to(src, 16)) ? 1 : 0;
    const int dv = (ld_dst % 4 == 0 && aligned_to(dst, 16)) ? 1 : 0;
    rows_h16_to_f32_kernel<<<grid_for(n * ((F + kVec - 1) / kVec), kBlock), kBlock, 0, as_stream(stream)>>>(
        static_cast<const uint16_t*>(src), ld_src, int(dtype), n, int(F), dst, ld_dst, sv, dv);
    TFGX_LAUNCH_CHECK("rows_h16_to_f32_kernel");
    return TFGX_OK;
}
