// Aggregation -> projection in ONE launch over a 16-BIT feature table (bf16 / fp16 storage, fp32 arithmetic):
// include/tfgx_fused_h16.h.  C = act( (reduce_{edges of r} w * x[col] (+ self_coef[r] * x[r]) [/ deg]) @ B + bias ).
//
// This is agg_gemm_kernel of tfgx_fused.hip with the producer walk of seg_reduce_h16_kernel (tfgx_reduce_h16.hip): one
// persistent 1024-thread workgroup per CU, B resident in LDS as far as it fits beside two TRANSPOSED 64-row tiles of the
// aggregate, units of the tile handed out from an LDS counter, the last arrivers of a tile multiplying it on the MFMA while
// the other waves reduce the next one.  What differs is the producer only: every lane gathers ONE 16-byte vector of 8
// elements per edge (a row touches half the 128-byte lines of its fp32 form), widens it in registers (bf16: a shift, fp16:
// v_cvt_f32_f16, both exact) and feeds the same in-order fp32 chain per output element — fmaf(w, x, acc) / acc + x in CSR
// edge order, then self_coef (the row's own features read from the 16-bit table), then the MEAN divide.  The call therefore
// returns, bit for bit, what tfgx_aggregate_gemm_f32 returns for the table widened to fp32 (C and the side output).
//
// Lane groups: lanes own 8 columns, so G = ceil(F / 8) rounded up to a power of two would be 1 .. 16.  A tile is cut into
// UNITS = 64 / (64 / G) = G units and the consumer jobs are taken by the LAST arrivers of a tile, so UNITS >= njobs must
// hold; njobs reaches 8 (N > 128).  G therefore never goes below 8: F <= 64 runs G = 8 (lanes past F read pad columns and
// store nothing), wider rows G = 16.  The alternative — a job count that follows G — would leave a tile of narrow rows to
// four or fewer consumer waves, the situation JB = 2 / eight jobs was introduced against in the fp32 kernel.
//
// The consumer below is a copy of tfgx_fused.hip's (that file's code generation must not move), less its developer
// switches; k order, accumulator layout and epilogue are the same expressions.
#include "tfgx_common.h"
#include "tfgx_mfma.h"
#include "../../include/tfgx_fused_h16.h"
#include <cstdio>
#include <cstring>
#include <type_traits>

namespace tfgx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTileRows = 64;
constexpr int kLda = kTileRows + 1;
constexpr int kBufs = 2;
constexpr int kFusedThreads = 1024;
constexpr int kVec = 8;      // elements per 16-byte vector of a 16-bit table
constexpr int kJB = 2;       // 32-column blocks per consumer job

struct FHArgs {
    const int32_t* row_ptr;
    const int32_t* col;
    const float* w;
    int64_t n_dst;
    const uint16_t* x;      // [n_src, ldx] 16-bit elements
    int64_t ldx;
    int32_t F;
    int32_t op;
    const float* self_coef;
    const int32_t* mean_count;
    const float* B;
    int64_t ldb;
    const float* bias;
    int32_t act;
    int32_t N;
    float* C;
    int64_t ldc;
    int32_t KP;        // F rounded up to even (the MFMA consumes two k per step)
    int32_t n_blocks;  // 32-column output blocks, rounded up to a multiple of 4
    int32_t LDW;       // NL + 8
    int64_t n_tiles;
    int32_t NL;        // columns of B resident in LDS (multiple of 64); columns >= NL: B operand from global
    float* agg;        // optional side output: the aggregated rows themselves, [n_dst, ld_agg] fp32, or NULL
    int64_t ld_agg;
    int32_t hub_threshold;
    int32_t n_hub;
    const int32_t* hub_rows;        // ascending
    const int32_t* hub_chunk_ptr;
    const float* hub_scratch;       // [chunks, F] fp32 chunk partials (written by tfgx_segment_reduce_h16 before this launch)
    const int32_t* row_order;
    const int32_t* hub_order_slot;
};

template <int G>
__device__ __forceinline__ int bcast_i(int v, int j) { return __shfl(v, j, G); }
template <int G>
__device__ __forceinline__ float bcast_f(float v, int j) { return __shfl(v, j, G); }

// 16-bit -> fp32 in registers (exact): the expressions of tfgx_reduce_h16.hip
template <int DT>
__device__ __forceinline__ void widen8(const uint4 r, float (&v)[kVec])
{
    const uint32_t u[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (DT == TFGX_DT_BF16) {
            v[2 * i] = __uint_as_float(u[i] << 16);
            v[2 * i + 1] = __uint_as_float(u[i] & 0xFFFF0000u);
        } else {
            v[2 * i] = float(__builtin_bit_cast(_Float16, static_cast<unsigned short>(u[i] & 0xFFFFu)));
            v[2 * i + 1] = float(__builtin_bit_cast(_Float16, static_cast<unsigned short>(u[i] >> 16)));
        }
    }
}

template <int DT, int G, bool WEIGHTED>
__global__ __launch_bounds__(kFusedThreads) void agg_gemm_h16_kernel(const FHArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Ws = lds;                                        // [KP][LDW]
    float* At = Ws + a.KP * a.LDW;                          // [kBufs][KP][kLda]
    int* ctrl = reinterpret_cast<int*>(At + kBufs * a.KP * kLda);   // [0] next unit | [1 + b] arrivals of buffer b | [1 + kBufs + b] done seq
    int* rowid = ctrl + 16;                                 // [kBufs][kTileRows]: the destination row of each tile slot (row_order)
    constexpr int RPW = 64 / G;                             // destination rows per wave step (one per lane group)
    constexpr int UNITS = kTileRows / RPW;
    constexpr int UNROLL = 8;
    static_assert(G == 8 || G == 16, "UNITS = G must cover the eight consumer jobs of a tile");
    const int tid = threadIdx.x, lane64 = tid & 63;
    const int lane = lane64 % G, grp = lane64 / G;

    for (int i = tid; i < a.KP * a.LDW; i += kFusedThreads) {
        const int k = i / a.LDW, n = i - k * a.LDW;
        Ws[i] = (k < a.F && n < a.N && n < a.NL) ? a.B[int64_t(k) * a.ldb + n] : 0.0f;
    }
    for (int i = tid; i < kBufs * a.KP * kLda; i += kFusedThreads) At[i] = 0.0f;      // rows k >= F stay zero for good
    if (tid < 16) ctrl[tid] = 0;                            // ([6 + b]: finished jobs of buffer b's tile)
    __syncthreads();

    const int64_t my_tiles = a.n_tiles > int64_t(blockIdx.x) ? (a.n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    const int64_t total_units = my_tiles * UNITS;
    // this lane's 8 columns: [c0, c0 + 8).  F % 4 == 0, so its halves [c0, c0 + 4) and [c0 + 4, c0 + 8) are valid or not as
    // a whole (F % 8 == 4 leaves the last valid lane half-valid).  Lanes past F read, branch-free and discarded, their OWN
    // vector of pad columns while it is inside the row stride, else the row's first vector (seg_reduce_h16_kernel).
    const int c0 = lane * kVec;
    const bool v_lo = c0 < a.F, v_hi = c0 + 4 < a.F;
    const int coff = (v_lo || int64_t(c0) + kVec <= a.ldx) ? c0 : 0;
    // fp32 rows of F columns (hub partials): a half past F re-reads the last valid vector (discarded)
    const int h_lo = v_lo ? c0 : a.F - 4, h_hi = v_hi ? c0 + 4 : a.F - 4;
    const int l31 = lane64 & 31, kh = lane64 >> 5;
    const bool vec_store = (a.N % 4 == 0) && (a.ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.C) & 15) == 0);      // wave-uniform
    const uint16_t* xb = a.x + coff;
    // element offset of a gathered row as ONE 32 x 32 -> 64-bit multiply: ids are non-negative int32, the stride fits 32 bits
    const uint32_t xl32 = uint32_t(a.ldx);
    auto row_off = [&](int i) { return uint64_t(uint32_t(i)) * xl32; };

    while (true) {
        int u = 0;
        if (lane64 == 0) u = atomicAdd(&ctrl[0], 1);
        u = __builtin_amdgcn_readfirstlane(u);
        if (u >= total_units) break;
        const int q = u / UNITS, slot = u - q * UNITS;      // tile sequence number inside this workgroup, unit inside the tile
        const int buf = q % kBufs;
        const int64_t tile = int64_t(blockIdx.x) + int64_t(q) * gridDim.x;
        const int m = slot * RPW + grp;                     // row inside the tile
        const int64_t ri = tile * kTileRows + m;
        const int64_t r = (a.row_order != nullptr && ri < a.n_dst) ? int64_t(a.row_order[ri]) : ri;

        // ---- producer: reduce destination row r (seg_reduce_h16_kernel's walk) -----------------------------------------
        float acc[kVec];
#pragma unroll
        for (int v = 0; v < kVec; ++v) acc[v] = 0.0f;
        if (r < a.n_dst) {
            const int s = a.row_ptr[r], e = a.row_ptr[r + 1];
            const bool hub = a.hub_threshold > 0 && e - s > a.hub_threshold;      // uniform inside the lane group
            int cj_next = 0;
            float wj_next = 0.0f;
            if (!hub && s + lane < e) {
                cj_next = a.col[s + lane];
                if constexpr (WEIGHTED) wj_next = a.w[s + lane];
            }
            if (hub) {
                // r is in the list: its slot.  Walk order by length puts the hub rows first, and the plan then hands over
                // their slots (one load, checked); otherwise a binary search
                int lo = (a.hub_order_slot != nullptr && a.row_order != nullptr && ri < a.n_hub) ? a.hub_order_slot[ri] : -1;
                if (lo < 0 || lo >= a.n_hub || a.hub_rows[lo] != int32_t(r)) {
                    int hi = a.n_hub - 1;
                    lo = 0;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (a.hub_rows[mid] < int32_t(r)) lo = mid + 1;
                        else hi = mid;
                    }
                }
                // fp32 chunk partials in chunk order, eight chunks in flight
                int c = a.hub_chunk_ptr[lo];
                const int c_end = a.hub_chunk_ptr[lo + 1];
                for (; c + UNROLL <= c_end; c += UNROLL) {
                    float pl[UNROLL][4], ph[UNROLL][4];
#pragma unroll
                    for (int t = 0; t < UNROLL; ++t) {
                        load_vec<4>(a.hub_scratch + int64_t(c + t) * a.F + h_lo, pl[t]);
                        load_vec<4>(a.hub_scratch + int64_t(c + t) * a.F + h_hi, ph[t]);
                    }
#pragma unroll
                    for (int t = 0; t < UNROLL; ++t)
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            acc[v] += pl[t][v];
                            acc[4 + v] += ph[t][v];
                        }
                }
                for (; c < c_end; ++c) {
                    float pl[4], ph[4];
                    load_vec<4>(a.hub_scratch + int64_t(c) * a.F + h_lo, pl);
                    load_vec<4>(a.hub_scratch + int64_t(c) * a.F + h_hi, ph);
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        acc[v] += pl[v];
                        acc[4 + v] += ph[v];
                    }
                }
            }
            for (int base = s; base < (hub ? s : e); base += G) {
                const int cj = cj_next;
                const float wj = wj_next;
                const int nxt = base + G + lane;
                if (nxt < e) {
                    cj_next = a.col[nxt];
                    if constexpr (WEIGHTED) wj_next = a.w[nxt];
                }
                const int cnt = min(G, e - base);
                // UNROLL independent 16-byte loads in flight per lane before the first FMA; the last, partial batch is ONE
                // batch too (masked): its missing slots repeat the last edge's load and drop their arithmetic by a select
                auto batch = [&](int j, auto masked) {
                    constexpr bool MASKED = decltype(masked)::value;
                    uint4 raw[UNROLL];
                    float ww[UNROLL];
#pragma unroll
                    for (int t = 0; t < UNROLL; ++t) {
                        const int idx = MASKED ? min(j + t, cnt - 1) : j + t;
                        const int c = bcast_i<G>(cj, idx);
                        if constexpr (WEIGHTED) ww[t] = bcast_f<G>(wj, idx);
                        raw[t] = *reinterpret_cast<const uint4*>(xb + row_off(c));
                    }
#pragma unroll
                    for (int t = 0; t < UNROLL; ++t) {
                        const bool live = !MASKED || j + t < cnt;
                        float xv[kVec];
                        widen8<DT>(raw[t], xv);
#pragma unroll
                        for (int v = 0; v < kVec; ++v) {
                            const float n = WEIGHTED ? fmaf(ww[t], xv[v], acc[v]) : acc[v] + xv[v];
                            acc[v] = live ? n : acc[v];
                        }
                    }
                };
                int j = 0;
                for (; j + UNROLL <= cnt; j += UNROLL) batch(j, std::false_type{});
                if (j < cnt) batch(j, std::true_type{});
            }
            if (a.self_coef) {                               // the implicit (r, r) edge appended after the row's edges
                const float sc = a.self_coef[r];
                float xs[kVec];
                widen8<DT>(*reinterpret_cast<const uint4*>(xb + uint64_t(r) * xl32), xs);
#pragma unroll
                for (int v = 0; v < kVec; ++v) acc[v] = fmaf(sc, xs[v], acc[v]);
            }
            if (a.op == TFGX_MEAN) {
                const int cnt = a.mean_count ? a.mean_count[r] : (e - s);
                const float divisor = float(cnt > 1 ? cnt : 1);
#pragma unroll
                for (int v = 0; v < kVec; ++v) acc[v] = acc[v] / divisor;
            }
        }
        if (a.agg != nullptr && r < a.n_dst) {                // training forward: the weight gradient needs the aggregate
            const float lo4[4] = {acc[0], acc[1], acc[2], acc[3]}, hi4[4] = {acc[4], acc[5], acc[6], acc[7]};
            if (v_lo) store_vec<4>(a.agg + r * a.ld_agg + c0, lo4);
            if (v_hi) store_vec<4>(a.agg + r * a.ld_agg + c0 + 4, hi4);
        }
        // ---- hand the row over: wait until the buffer's previous tile (q - kBufs) has been multiplied, store transposed
        if (q >= kBufs) {
            volatile int* done = ctrl + 1 + kBufs + buf;
            while (*done < q - kBufs + 1) __builtin_amdgcn_s_sleep(1);
            __threadfence_block();
        }
        float* ab = At + buf * a.KP * kLda;
        if (v_lo) {
#pragma unroll
            for (int v = 0; v < 4; ++v) ab[(c0 + v) * kLda + m] = acc[v];
        }
        if (v_hi) {
#pragma unroll
            for (int v = 4; v < kVec; ++v) ab[(c0 + v) * kLda + m] = acc[v];
        }
        if (a.row_order != nullptr && lane == 0) rowid[buf * kTileRows + m] = ri < a.n_dst ? int(r) : -1;
        __threadfence_block();
        int arrived = 0;
        if (lane64 == 0) arrived = atomicAdd(&ctrl[1 + buf], 1);
        arrived = __builtin_amdgcn_readfirstlane(arrived);
        constexpr int JB = kJB;
        const int njobs = 2 * (a.n_blocks / JB);             // 4 (N <= 128) or 8: never more than UNITS = G >= 8
        if (arrived < UNITS - njobs) continue;

        // ---- consumers: the last arrivers of tile q each multiply ONE 32-row x (32 JB)-column block of it (the last one at
        // once, the ones before it as soon as the tile is complete) -> C[tile rows, :] = act(At^T @ Ws + bias)
        const int job = UNITS - 1 - arrived;                 // the last arriver takes block 0, the one before it block 1, ...
        if (job > 0) {
            volatile int* arr = ctrl + 1 + buf;
            while (*arr < UNITS) __builtin_amdgcn_s_sleep(1);
        }
        __threadfence_block();
        const int mb = job & 1, nb0 = (job >> 1) * JB;
        {
            f32x16 c4[JB];
#pragma unroll
            for (int jb = 0; jb < JB; ++jb)
#pragma unroll
                for (int t = 0; t < 16; ++t) c4[jb][t] = 0.0f;
            const float* ap = ab + kh * kLda + mb * 32 + l31;
            const int pairs = a.KP / 2;
            int pr = 0;
            if (nb0 * 32 < a.NL) {
                // B resident in LDS.  KU k-pairs per step: all (1 + JB) * KU LDS reads of a step are issued before its
                // JB * KU MFMAs
                const float* bp = Ws + kh * a.LDW + nb0 * 32 + l31;
                constexpr int KU = 4;
                for (; pr + KU <= pairs; pr += KU) {
                    float av[KU], bv[KU][JB];
#pragma unroll
                    for (int t = 0; t < KU; ++t) {
                        av[t] = ap[(2 * (pr + t)) * kLda];
#pragma unroll
                        for (int jb = 0; jb < JB; ++jb) bv[t][jb] = bp[(2 * (pr + t)) * a.LDW + jb * 32];
                    }
                    __builtin_amdgcn_sched_barrier(0);      // left alone the scheduler sinks every read next to its MFMA
#pragma unroll
                    for (int t = 0; t < KU; ++t)
#pragma unroll
                        for (int jb = 0; jb < JB; ++jb)
                            c4[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[t][jb], c4[jb], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                for (; pr < pairs; ++pr) {
                    const float av = ap[(2 * pr) * kLda];
                    float bv[JB];
#pragma unroll
                    for (int jb = 0; jb < JB; ++jb) bv[jb] = bp[(2 * pr) * a.LDW + jb * 32];
#pragma unroll
                    for (int jb = 0; jb < JB; ++jb) c4[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[jb], c4[jb], 0, 0, 0);
                }
            } else {
                // B columns past the resident ones: the operand comes from global memory (L2: every workgroup re-reads the
                // same <= 128 KB for every tile).  Lane (l31, kh) reads B[2 pr + kh][col]; KG k-pairs = JB * KG loads in
                // flight per wave before the first MFMA of the step.  Columns >= N read column N - 1 (never stored).
                const float* gp[JB];
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) {
                    const int gn = (nb0 + jb) * 32 + l31;
                    gp[jb] = a.B + int64_t(kh) * a.ldb + (gn < a.N ? gn : a.N - 1);
                }
                constexpr int KG = 8;
                for (; pr + KG <= pairs; pr += KG) {
                    float av[KG], bv[KG][JB];
#pragma unroll
                    for (int t = 0; t < KG; ++t)
#pragma unroll
                        for (int jb = 0; jb < JB; ++jb) bv[t][jb] = gp[jb][int64_t(2 * (pr + t)) * a.ldb];
#pragma unroll
                    for (int t = 0; t < KG; ++t) av[t] = ap[(2 * (pr + t)) * kLda];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int t = 0; t < KG; ++t)
#pragma unroll
                        for (int jb = 0; jb < JB; ++jb)
                            c4[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[t][jb], c4[jb], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                for (; pr < pairs; ++pr) {
                    const float av = ap[(2 * pr) * kLda];
                    float bv[JB];
#pragma unroll
                    for (int jb = 0; jb < JB; ++jb) bv[jb] = (2 * pr + kh < a.F) ? gp[jb][int64_t(2 * pr) * a.ldb] : 0.0f;
#pragma unroll
                    for (int jb = 0; jb < JB; ++jb) c4[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[jb], c4[jb], 0, 0, 0);
                }
            }
            // D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).  Two phases on purpose: bias +
            // activation IN PLACE first, then every store reads its own accumulator register
#pragma unroll
            for (int jb = 0; jb < JB; ++jb) {
                const int gn = (nb0 + jb) * 32 + l31;
                const float bv = (a.bias && gn < a.N) ? a.bias[gn] : 0.0f;
#pragma unroll
                for (int t = 0; t < 16; ++t) c4[jb][t] = apply_act(c4[jb][t] + bv, a.act);
            }
            const int64_t row0 = tile * kTileRows + mb * 32 + 4 * kh;
            const bool full = tile * kTileRows + kTileRows <= a.n_dst;
            if (a.row_order != nullptr && !vec_store) {     // walk order without 16-byte stores (odd N / unaligned C)
                const int* rid = rowid + buf * kTileRows + mb * 32 + 4 * kh;
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) {
                    const int gn = (nb0 + jb) * 32 + l31;
                    if (gn >= a.N) continue;
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        const int rr = rid[(t & 3) + 8 * (t >> 2)];
                        if (rr >= 0) __builtin_nontemporal_store(c4[jb][t], a.C + int64_t(rr) * a.ldc + gn);
                    }
                }
            } else if (vec_store && (full || a.row_order != nullptr)) {
                // 16-byte stores through a quad transpose of the accumulators (tfgx_mfma.h): lane i of a quad ends with row
                // 8 g + i + 4 kh, columns 4 q .. 4 q + 3
                const int qi = lane64 & 3, qc = (l31 >> 2) * 4;
                typedef float f32x4s __attribute__((ext_vector_type(4)));
                int64_t roff[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int sl = mb * 32 + 8 * g + qi + 4 * kh;
                    const int64_t rr = a.row_order != nullptr ? int64_t(rowid[buf * kTileRows + sl]) : tile * kTileRows + sl;
                    roff[g] = rr >= 0 ? rr * a.ldc : int64_t(-1);
                }
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) {
                    float r4[4][4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {          // (every lane takes part in the quad permutes)
#pragma unroll
                        for (int k = 0; k < 4; ++k) r4[g][k] = c4[jb][4 * g + k];
                        quad_transpose4(r4[g], lane64);
                    }
                    const int gn = (nb0 + jb) * 32 + qc;
                    if (gn < a.N) {
#pragma unroll
                        for (int g = 0; g < 4; ++g)
                            if (roff[g] >= 0)
                                __builtin_nontemporal_store(f32x4s{r4[g][0], r4[g][1], r4[g][2], r4[g][3]},
                                                            reinterpret_cast<f32x4s*>(a.C + roff[g] + gn));
                    }
                }
            } else {
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) {
                    const int gn = (nb0 + jb) * 32 + l31;
                    if (gn >= a.N) continue;
                    float* cp = a.C + row0 * a.ldc + gn;
                    if (full) {
#pragma unroll
                        for (int t = 0; t < 16; ++t)
                            __builtin_nontemporal_store(c4[jb][t], cp + int64_t((t & 3) + 8 * (t >> 2)) * a.ldc);
                    } else {
#pragma unroll
                        for (int t = 0; t < 16; ++t) {
                            const int dr = (t & 3) + 8 * (t >> 2);
                            if (row0 + dr < a.n_dst) cp[int64_t(dr) * a.ldc] = c4[jb][t];
                        }
                    }
                }
            }
        }
        __threadfence_block();
        int fin = 0;
        if (lane64 == 0) fin = atomicAdd(&ctrl[6 + buf], 1);
        fin = __builtin_amdgcn_readfirstlane(fin);
        if (fin == njobs - 1) {
            // the last job to finish hands the buffer back (wave-uniform branch; every lane stores the same values)
            ctrl[1 + buf] = 0;
            ctrl[6 + buf] = 0;
            __threadfence_block();
            *reinterpret_cast<volatile int*>(ctrl + 1 + kBufs + buf) = q + 1;
        }
    }
}

// LDS budget: the arithmetic of tfgx_fused.hip (the envelope itself is tfgx_aggregate_gemm_fits, not restated here)
inline size_t fused_lds_bytes(int kp, int ldw)
{
    return sizeof(float) * (size_t(kp) * ldw + size_t(kBufs) * kp * kLda) + sizeof(int) * (16 + kBufs * kTileRows);
}

constexpr size_t kFusedLdsLimit = 160 * 1024;

inline int fused_resident_cols(int kp, int np)
{
    for (int nl = np; nl >= 64; nl -= 64)
        if (fused_lds_bytes(kp, nl + 8) <= kFusedLdsLimit) return nl;
    return 0;
}

inline int group_lanes(int64_t F) { return F <= 64 ? 8 : 16; }      // the ONE place G is decided (launch and describe)

// The host checks the launch and describe share; every refusal names the member.
int check_fused_h16(const char* fn, const tfgx_reduce_args* p, int32_t x_dtype, int64_t N)
{
#define FH_REQUIRE(cond, msg)                        \
    do {                                             \
        if (!(cond)) {                               \
            set_error("%s: %s", fn, msg);            \
            return TFGX_ERR_INVALID_ARG;             \
        }                                            \
    } while (0)
    FH_REQUIRE(p != nullptr, "args is null");
    FH_REQUIRE(x_dtype == TFGX_DT_BF16 || x_dtype == TFGX_DT_F16, "bad x_dtype (TFGX_DT_BF16 or TFGX_DT_F16)");
    FH_REQUIRE(p->op == TFGX_SUM || p->op == TFGX_MEAN, "op: sum / mean only (TFGX_MAX is refused)");
    FH_REQUIRE(tfgx_aggregate_gemm_fits(p->F, N) == 1, "F / N: shape not supported (tfgx_aggregate_gemm_fits)");
    FH_REQUIRE(p->n_dst >= 0 && p->n_dst < (int64_t(1) << 31), "bad n_dst");
    FH_REQUIRE(p->x_tail == nullptr, "x_tail: the split-row layout is not supported on a 16-bit table");
    FH_REQUIRE(p->edge_tail == nullptr, "edge_tail: the split-row layout is not supported on a 16-bit table");
    FH_REQUIRE(p->verify == 0, "verify: the verified layout is not supported on a 16-bit table");
    FH_REQUIRE(p->track == nullptr, "track: plain aggregation only");
    FH_REQUIRE(!p->accumulate, "accumulate: plain aggregation only");
    FH_REQUIRE(p->add_x == nullptr, "add_x: plain aggregation only");
    FH_REQUIRE(p->ldx % kVec == 0, "ldx: rows of a 16-bit table must be 16-byte aligned (ldx % 8 == 0)");
    FH_REQUIRE(p->ldx >= (p->F + kVec - 1) / kVec * kVec && p->ldx < (int64_t(1) << 31), "ldx: must hold roundup8(F) elements and be below 2^31");
    FH_REQUIRE(aligned_to(p->x, 16), "x: rows of a 16-bit table must be 16-byte aligned (misaligned base)");
    if (p->n_dst == 0) return TFGX_OK;
    FH_REQUIRE(p->row_begin && p->row_end == p->row_begin + 1 && p->rp_stride == 1,
               "row_begin / row_end / rp_stride: needs a plain CSR (row_ptr, row_ptr + 1, stride 1), no explicit spans");
    FH_REQUIRE(p->x != nullptr, "x: null pointer");
    FH_REQUIRE(p->out == nullptr || (p->ldo >= p->F && p->ldo % 4 == 0 && aligned_to(p->out, 16)),
               "out / ldo: side output of the aggregate: rows of >= F floats, 16-byte aligned");
    if (p->hub_threshold > 0 && p->n_hub_rows > 0)
        FH_REQUIRE(p->hub_rows && p->hub_chunk_ptr && p->hub_chunk_begin && p->hub_chunk_end && p->hub_scratch &&
                       p->n_hub_chunks > 0 && p->n_hub_rows < (int64_t(1) << 31) && aligned_to(p->hub_scratch, 16),
                   "hub_rows: given without chunk lists / 16-byte aligned scratch");
#undef FH_REQUIRE
    return TFGX_OK;
}

template <int DT, int G, bool WEIGHTED>
int launch_one(const FHArgs& a, int dev, int64_t wgs, size_t lds_bytes, hipStream_t stream)
{
    constexpr int kMaxDev = 64;
    static bool attr_set[kMaxDev] = {false};      // per DEVICE and instantiation: the dynamic-LDS attribute
    if (!attr_set[dev]) {
        TFGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(agg_gemm_h16_kernel<DT, G, WEIGHTED>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, int(kFusedLdsLimit)));
        attr_set[dev] = true;
    }
    agg_gemm_h16_kernel<DT, G, WEIGHTED><<<dim3(unsigned(wgs)), dim3(kFusedThreads), lds_bytes, stream>>>(a);
    TFGX_LAUNCH_CHECK("agg_gemm_h16_kernel");
    return TFGX_OK;
}

template <int DT>
int launch_dt(const FHArgs& a, int g, bool weighted, int dev, int64_t wgs, size_t lds_bytes, hipStream_t stream)
{
    if (g == 8) return weighted ? launch_one<DT, 8, true>(a, dev, wgs, lds_bytes, stream) : launch_one<DT, 8, false>(a, dev, wgs, lds_bytes, stream);
    return weighted ? launch_one<DT, 16, true>(a, dev, wgs, lds_bytes, stream) : launch_one<DT, 16, false>(a, dev, wgs, lds_bytes, stream);
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_fused_h16_version(void) { return TFGX_FUSED_H16_ABI_VERSION; }

extern "C" int tfgx_aggregate_gemm_h16_describe(const tfgx_reduce_args* p, int32_t x_dtype, int64_t N, char* buf, size_t buf_bytes)
{
    TFGX_REQUIRE(buf != nullptr && buf_bytes > 0, "null buffer");
    buf[0] = '\0';
    const int rc = check_fused_h16(__func__, p, x_dtype, N);
    if (rc != TFGX_OK) return rc;
    char name[96];
    const int len = snprintf(name, sizeof(name), "agg_gemm_h16_kernel<%d, %d, %s>", int(x_dtype), group_lanes(p->F),
                             p->w ? "true" : "false");
    TFGX_REQUIRE(size_t(len) + 1 <= buf_bytes, "buffer too small");
    memcpy(buf, name, size_t(len) + 1);
    return TFGX_OK;
}

extern "C" int tfgx_aggregate_gemm_h16(const tfgx_reduce_args* p, int32_t x_dtype, const float* B, int64_t ldb, const float* bias,
                                       int32_t act, float* C, int64_t ldc, int64_t N, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    const int rc0 = check_fused_h16(__func__, p, x_dtype, N);
    if (rc0 != TFGX_OK) return rc0;
    TFGX_REQUIRE(act == TFGX_ACT_NONE || act == TFGX_ACT_RELU, "bad act");
    if (p->n_dst == 0) return TFGX_OK;
    TFGX_REQUIRE(B && C, "B / C: null pointer");          // (col may be NULL for a graph without edges)
    TFGX_REQUIRE(ldb >= N && ldc >= N, "ldb / ldc: leading dimension < N");
    const bool use_hub = p->hub_threshold > 0 && p->n_hub_rows > 0;
    if (use_hub) {
        // chunk partials first: every chunk is reduced like an ordinary row of the 16-bit table into the fp32 hub_scratch
        // (tfgx_segment_reduce_h16 — the bits tfgx_segment_reduce_f32 leaves there for the widened table)
        tfgx_reduce_args c = *p;
        c.row_begin = p->hub_chunk_begin; c.row_end = p->hub_chunk_end; c.rp_stride = 1;
        c.n_dst = p->n_hub_chunks; c.out = p->hub_scratch; c.ldo = p->F;
        c.op = TFGX_SUM; c.act = TFGX_ACT_NONE; c.accumulate = 0;
        c.self_coef = nullptr; c.bias = nullptr; c.add_x = nullptr; c.mean_count = nullptr;
        c.hub_threshold = 0; c.hub_rows = nullptr; c.hub_chunk_ptr = nullptr; c.hub_chunk_begin = nullptr;
        c.hub_chunk_end = nullptr; c.n_hub_rows = 0; c.n_hub_chunks = 0; c.hub_scratch = nullptr;
        c.row_order = nullptr;          // (a walk order names DESTINATION rows; the chunk launch walks chunks)
        c.hub_order_slot = nullptr;
        const int rc = tfgx_segment_reduce_h16(&c, x_dtype, TFGX_DT_F32, stream_);
        if (rc != TFGX_OK) return rc;
    }
    FHArgs a;
    a.hub_threshold = use_hub ? p->hub_threshold : 0;
    a.n_hub = use_hub ? int32_t(p->n_hub_rows) : 0;
    a.hub_rows = p->hub_rows; a.hub_chunk_ptr = p->hub_chunk_ptr; a.hub_scratch = p->hub_scratch;
    a.row_order = p->row_order;
    a.hub_order_slot = use_hub ? p->hub_order_slot : nullptr;
    a.row_ptr = p->row_begin; a.col = p->col; a.w = p->w; a.n_dst = p->n_dst;
    a.x = static_cast<const uint16_t*>(static_cast<const void*>(p->x)); a.ldx = p->ldx; a.F = int32_t(p->F);
    a.op = p->op; a.self_coef = p->self_coef; a.mean_count = p->mean_count;
    a.B = B; a.ldb = ldb; a.bias = bias; a.act = act; a.N = int32_t(N); a.C = C; a.ldc = ldc;
    a.agg = static_cast<float*>(p->out); a.ld_agg = p->ldo;
    a.KP = int32_t((p->F + 1) / 2 * 2);
    a.n_blocks = int32_t((N + 127) / 128) * 4;          // 32-column blocks, in groups of four (columns >= N are zero in LDS)
    a.NL = fused_resident_cols(a.KP, 32 * a.n_blocks);
    a.LDW = a.NL + 8;
    a.n_tiles = (p->n_dst + kTileRows - 1) / kTileRows;
    constexpr int kMaxDev = 64;
    static int cus_of[kMaxDev] = {0};
    int dev = 0;
    TFGX_HIP_CHECK(hipGetDevice(&dev));
    TFGX_REQUIRE(dev >= 0 && dev < kMaxDev, "device ordinal out of range");
    if (cus_of[dev] == 0) {
        hipDeviceProp_t prop;
        TFGX_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
        cus_of[dev] = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    const int cus = cus_of[dev];
    const size_t lds_bytes = fused_lds_bytes(a.KP, a.LDW);
    const int64_t wgs = a.n_tiles < cus ? a.n_tiles : cus;
    hipStream_t stream = as_stream(stream_);
    const bool weighted = p->w != nullptr;
    const int g = group_lanes(p->F);
    if (x_dtype == TFGX_DT_BF16) return launch_dt<TFGX_DT_BF16>(a, g, weighted, dev, wgs, lds_bytes, stream);
    return launch_dt<TFGX_DT_F16>(a, g, weighted, dev, wgs, lds_bytes, stream);
}
