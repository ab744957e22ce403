// Set2Set's two hot paths (include/tfgx_set2set.h): the per-graph attention readout with an online softmax, and a stateful
// sequence LSTM; each with its backward.
//
// Reference: nn/pool/set2set.py:28-40 (per iteration: lstm over the query sequence; gather, multiply, row sum, a three-op
// segment_softmax, multiply, segment sum) and nn/kernel/segment.py:26-33.
//
// Attention.  A WAVE owns one chunk: up to kChunk consecutive CSR rows of one graph.  A row is spread over LG lanes (LG a
// power of two, each lane VEC * KV features), so a wave reads 64 / LG rows side by side and kRows batches of them per loop
// trip; the dot product meets in an xor tree over the LG lanes and the lane groups' (m, s, r) states meet in an xor tree at
// the end.  Both trees depend on F and the alignment only, never on the data.
// Work items: w < G is chunk 0 of graph w.  Chunk k >= 1 of a graph starts at CSR position row_ptr[g] + k * kChunk and is
// owned by item G + (that position / kChunk): two such chunks never share a slot (the previous chunk of the same graph
// covers the kChunk positions before the start), so ceil(N / kChunk) slot items cover every cut graph and the owner of a
// slot is found with one binary search in row_ptr — no prefix sum, no host read.  The merge launch runs over the slots
// too: the block whose slot holds chunk 1 of a graph merges that graph, chunk by chunk.
//
// Sequence LSTM.  A workgroup of 4U threads owns ROWS batch rows for all T steps: thread j accumulates gate column j of
// h_{t-1} @ R (h broadcast from LDS, R from LDS when resident, else L2), the activated gates meet in LDS, threads u < U
// update c and h.  Backward: threads u < U rebuild dz from the saved gates, then every wave takes 16 rows u of R and
// reduces dh_{t-1}[u] = <dz_t, R[u, :]> over its lanes in a fixed xor tree.
#include "tfgx_common.h"
#include "../../include/tfgx_set2set.h"

namespace tfgx {
namespace {

constexpr int kChunk = TFGX_SET2SET_CHUNK_ROWS;
constexpr int kRows = 4;                            // row batches in flight per lane group
constexpr int kWaves = kBlock / kWave;
constexpr size_t kLdsLimit = 160 * 1024;
constexpr int64_t kInt32Max = (int64_t(1) << 31) - 1;
constexpr float kEps = 1e-8f;

// ---------------------------------------------------------------------------------------------------------------------------
// work items
struct Item {
    int g;          // graph, -1: nothing to do
    int k;          // chunk of the graph
    int beg, end;   // CSR positions of the chunk
    int gbeg, gend; // CSR positions of the graph
    int bad;
};

__device__ __forceinline__ bool span_ok(int64_t b, int64_t e, int64_t N) { return b >= 0 && e >= b && e <= N; }

// wave-uniform: every lane computes the same item
__device__ __forceinline__ Item find_item(const int32_t* __restrict__ row_ptr, int64_t G, int64_t N, int64_t w)
{
    Item it;
    it.g = -1;
    it.k = 0;
    it.beg = it.end = it.gbeg = it.gend = 0;
    it.bad = 0;
    if (w < G) {
        const int64_t b = row_ptr[w], e = row_ptr[w + 1];
        it.g = int(w);
        if (!span_ok(b, e, N)) {
            it.bad = 1;
            return it;      // an empty graph
        }
        it.gbeg = it.beg = int(b);
        it.gend = int(e);
        it.end = int(e - b > kChunk ? b + kChunk : e);
        return it;
    }
    const int64_t pos = (w - G) * kChunk;
    if (pos >= N) return it;
    // the graph that holds CSR position pos: the last g with row_ptr[g] <= pos
    int64_t lo = 0, hi = G;      // row_ptr[lo] <= pos is assumed (row_ptr[0] = 0), answer in [lo, hi)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (int64_t(row_ptr[mid]) <= pos) lo = mid;
        else hi = mid;
    }
    const int64_t b = row_ptr[lo], e = row_ptr[lo + 1];
    if (!span_ok(b, e, N) || b > pos || e <= pos) return it;      // chunk 0 of that graph reports a bad span
    const int64_t k = (pos - b + kChunk - 1) / kChunk;
    const int64_t s = b + k * kChunk;
    if (k < 1 || s >= e) return it;
    it.g = int(lo);
    it.k = int(k);
    it.gbeg = int(b);
    it.gend = int(e);
    it.beg = int(s);
    it.end = int(e - s > kChunk ? s + kChunk : e);
    return it;
}

__device__ __forceinline__ float weight_of(float m, float M) { return m == -INFINITY ? 0.0f : expf(m - M); }

// workspace: ms0 [G][2] (chunk 0 of a cut graph), slot_ms [nslots][2], slot_r [nslots][F]
struct Workspace {
    float* ms0;
    float* slot_ms;
    float* slot_r;
};

inline int64_t slots_of(int64_t N) { return N > kChunk ? (N + kChunk - 1) / kChunk : 0; }

inline Workspace carve(void* ws, int64_t G, int64_t nslots)
{
    Workspace w;
    w.ms0 = static_cast<float*>(ws);
    w.slot_ms = w.ms0 + 2 * G;
    w.slot_r = w.slot_ms + 2 * nslots;
    return w;
}

// ---------------------------------------------------------------------------------------------------------------------------
// attention forward
template <int VEC, int KV>
__global__ void __launch_bounds__(kBlock) attend_forward_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ node,
                                                                int64_t G, int64_t N, int64_t nslots, const float* __restrict__ x,
                                                                int64_t ldx, int F, int lg, const float* __restrict__ q, int64_t ldq,
                                                                float* __restrict__ r, int64_t ldr, float* __restrict__ stats,
                                                                Workspace ws, int32_t* __restrict__ flag)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t w = int64_t(blockIdx.x) * kWaves + wave;
    if (w >= G + nslots) return;
    const Item it = find_item(row_ptr, G, N, w);
    int bad = it.bad;
    if (it.g < 0) return;
    const int LG = 1 << lg, sub = lane & (LG - 1), grp = lane >> lg, RP = kWave >> lg;

    int col[KV];
    float qv[KV][VEC], racc[KV][VEC];
#pragma unroll
    for (int kv = 0; kv < KV; ++kv) {
        col[kv] = (kv * LG + sub) * VEC;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            qv[kv][v] = col[kv] + v < F ? q[int64_t(it.g) * ldq + col[kv] + v] : 0.0f;
            racc[kv][v] = 0.0f;
        }
    }
    float m = -INFINITY, s = 0.0f;

    for (int64_t p0 = it.beg; p0 < it.end; p0 += RP * kRows) {
        bool ok[kRows];
        float xv[kRows][KV][VEC], e[kRows];
#pragma unroll
        for (int b = 0; b < kRows; ++b) {
            const int64_t p = p0 + b * RP + grp;
            ok[b] = false;
            int64_t idx = 0;
            if (p < it.end) {
                idx = node[p];
                ok[b] = idx >= 0 && idx < N;
                bad |= !ok[b];
            }
            const float* xr = x + idx * ldx;
            e[b] = 0.0f;
#pragma unroll
            for (int kv = 0; kv < KV; ++kv) {
                if (ok[b] && col[kv] < F) load_vec<VEC>(xr + col[kv], xv[b][kv]);
                else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) xv[b][kv][v] = 0.0f;
                }
#pragma unroll
                for (int v = 0; v < VEC; ++v) e[b] = fmaf(xv[b][kv][v], qv[kv][v], e[b]);
            }
        }
        for (int o = LG >> 1; o > 0; o >>= 1) {
#pragma unroll
            for (int b = 0; b < kRows; ++b) e[b] += __shfl_xor(e[b], o);
        }
        float mn = m;
#pragma unroll
        for (int b = 0; b < kRows; ++b)
            if (ok[b]) mn = fmaxf(mn, e[b]);
        if (mn != -INFINITY) {
            const float sc = weight_of(m, mn);
            s *= sc;
#pragma unroll
            for (int kv = 0; kv < KV; ++kv)
#pragma unroll
                for (int v = 0; v < VEC; ++v) racc[kv][v] *= sc;
#pragma unroll
            for (int b = 0; b < kRows; ++b) {
                const float p = ok[b] ? expf(e[b] - mn) : 0.0f;
                s += p;
#pragma unroll
                for (int kv = 0; kv < KV; ++kv)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) racc[kv][v] = fmaf(p, xv[b][kv][v], racc[kv][v]);
            }
            m = mn;
        }
    }
    // the lane groups' states meet: group 0 ends with ((g0 + g1) + (g2 + g3)) + ...
    for (int o = LG; o < kWave; o <<= 1) {
        const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        const float M = fmaxf(m, m2);
        const float a = weight_of(m, M), b2 = weight_of(m2, M);
        s = s * a + s2 * b2;
#pragma unroll
        for (int kv = 0; kv < KV; ++kv)
#pragma unroll
            for (int v = 0; v < VEC; ++v) racc[kv][v] = racc[kv][v] * a + __shfl_xor(racc[kv][v], o) * b2;
        m = M;
    }
    if (flag != nullptr && __any(bad) && lane == 0) atomicOr(flag, 1);
    if (grp != 0) return;
    const bool cut = it.gend - it.gbeg > kChunk;
    if (!cut) {
        const float D = s + kEps;
#pragma unroll
        for (int kv = 0; kv < KV; ++kv)
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                if (col[kv] + v < F) r[int64_t(it.g) * ldr + col[kv] + v] = racc[kv][v] / D;
        if (stats != nullptr && sub == 0) {
            stats[2 * int64_t(it.g)] = m == -INFINITY ? 0.0f : m;
            stats[2 * int64_t(it.g) + 1] = D;
        }
        return;
    }
    // a cut graph: chunk 0 parks its partial in r's own row, the others in their slot
    const int64_t slot = it.beg / kChunk;
    float* dst = it.k == 0 ? r + int64_t(it.g) * ldr : ws.slot_r + slot * F;
    float* ms = it.k == 0 ? ws.ms0 + 2 * int64_t(it.g) : ws.slot_ms + 2 * slot;
#pragma unroll
    for (int kv = 0; kv < KV; ++kv)
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            if (col[kv] + v < F) dst[col[kv] + v] = racc[kv][v];
    if (sub == 0) {
        ms[0] = m;
        ms[1] = s;
    }
}

// one block per slot; the block whose slot holds chunk 1 of a graph merges that graph's chunks in chunk order
__global__ void __launch_bounds__(kBlock) attend_merge_kernel(const int32_t* __restrict__ row_ptr, int64_t G, int64_t N, int F,
                                                              float* __restrict__ r, int64_t ldr, float* __restrict__ stats,
                                                              Workspace ws)
{
    __shared__ float red[kBlock];
    const Item it = find_item(row_ptr, G, N, G + blockIdx.x);
    if (it.g < 0 || it.k != 1) return;
    const int tid = threadIdx.x;
    const int nch = (it.gend - it.gbeg + kChunk - 1) / kChunk;
    const int64_t g = it.g;
    // the maximum is order-free
    float M = tid == 0 ? ws.ms0[2 * g] : -INFINITY;
    for (int k = 1 + tid; k < nch; k += kBlock) M = fmaxf(M, ws.slot_ms[2 * ((int64_t(it.gbeg) + int64_t(k) * kChunk) / kChunk)]);
    red[tid] = M;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]);
        __syncthreads();
    }
    M = red[0];
    // chunk weights exp(m_k - M), computed once per tile of kBlock chunks and shared through LDS; s and r are then summed
    // chunk by chunk (every thread repeats the short sum of s, a thread owns the features f = tid, tid + kBlock, ...)
    __shared__ float wt[kBlock], st[kBlock];
    __shared__ int64_t sl[kBlock];
    constexpr int kFeat = TFGX_SET2SET_MAX_FEATURES / kBlock;
    float s = 0.0f, acc[kFeat];
#pragma unroll
    for (int i = 0; i < kFeat; ++i) acc[i] = 0.0f;
    for (int k0 = 0; k0 < nch; k0 += kBlock) {
        __syncthreads();
        const int k = k0 + tid;
        if (k < nch) {
            const int64_t slot = (int64_t(it.gbeg) + int64_t(k) * kChunk) / kChunk;
            const float* ms = k == 0 ? ws.ms0 + 2 * g : ws.slot_ms + 2 * slot;
            wt[tid] = weight_of(ms[0], M);
            st[tid] = ms[1];
            sl[tid] = slot;
        }
        __syncthreads();
        const int cnt = nch - k0 < kBlock ? nch - k0 : kBlock;
        for (int j = 0; j < cnt; ++j) {
            s += st[j] * wt[j];
            const float* src = k0 + j == 0 ? r + g * ldr : ws.slot_r + sl[j] * F;
#pragma unroll
            for (int i = 0; i < kFeat; ++i) {
                const int f = tid + i * kBlock;
                if (f < F) acc[i] += src[f] * wt[j];
            }
        }
    }
    const float D = s + kEps;
#pragma unroll
    for (int i = 0; i < kFeat; ++i) {
        const int f = tid + i * kBlock;
        if (f < F) r[g * ldr + f] = acc[i] / D;
    }
    if (stats != nullptr && tid == 0) {
        stats[2 * g] = M == -INFINITY ? 0.0f : M;
        stats[2 * g + 1] = D;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// attention backward
template <int VEC, int KV>
__global__ void __launch_bounds__(kBlock) attend_backward_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ node,
                                                                 int64_t G, int64_t N, int64_t nslots, const float* __restrict__ x,
                                                                 int64_t ldx, int F, int lg, const float* __restrict__ q, int64_t ldq,
                                                                 const float* __restrict__ r, int64_t ldr,
                                                                 const float* __restrict__ stats, const float* __restrict__ d_r,
                                                                 int64_t ldg, float* __restrict__ d_x, int64_t lddx,
                                                                 float* __restrict__ d_q, int64_t lddq, float* __restrict__ slot_dq)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t w = int64_t(blockIdx.x) * kWaves + wave;
    if (w >= G + nslots) return;
    const Item it = find_item(row_ptr, G, N, w);
    if (it.g < 0) return;
    const int LG = 1 << lg, sub = lane & (LG - 1), grp = lane >> lg, RP = kWave >> lg;
    const int64_t g = it.g;

    int col[KV];
    float qv[KV][VEC], gv[KV][VEC], dq[KV][VEC];
    float c = 0.0f;
#pragma unroll
    for (int kv = 0; kv < KV; ++kv) {
        col[kv] = (kv * LG + sub) * VEC;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const bool in = col[kv] + v < F;
            qv[kv][v] = in ? q[g * ldq + col[kv] + v] : 0.0f;
            gv[kv][v] = in ? d_r[g * ldg + col[kv] + v] : 0.0f;
            c = fmaf(gv[kv][v], in ? r[g * ldr + col[kv] + v] : 0.0f, c);
            dq[kv][v] = 0.0f;
        }
    }
    for (int o = LG >> 1; o > 0; o >>= 1) c += __shfl_xor(c, o);
    const float m = stats[2 * g], D = stats[2 * g + 1];

    for (int64_t p0 = it.beg; p0 < it.end; p0 += RP * kRows) {
        bool ok[kRows];
        int64_t idx[kRows];
        float xv[kRows][KV][VEC], e[kRows], da[kRows];
#pragma unroll
        for (int b = 0; b < kRows; ++b) {
            const int64_t p = p0 + b * RP + grp;
            ok[b] = false;
            idx[b] = 0;
            if (p < it.end) {
                idx[b] = node[p];
                ok[b] = idx[b] >= 0 && idx[b] < N;
            }
            const float* xr = x + idx[b] * ldx;
            e[b] = da[b] = 0.0f;
#pragma unroll
            for (int kv = 0; kv < KV; ++kv) {
                if (ok[b] && col[kv] < F) load_vec<VEC>(xr + col[kv], xv[b][kv]);
                else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) xv[b][kv][v] = 0.0f;
                }
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    e[b] = fmaf(xv[b][kv][v], qv[kv][v], e[b]);
                    da[b] = fmaf(xv[b][kv][v], gv[kv][v], da[b]);
                }
            }
        }
        for (int o = LG >> 1; o > 0; o >>= 1) {
#pragma unroll
            for (int b = 0; b < kRows; ++b) {
                e[b] += __shfl_xor(e[b], o);
                da[b] += __shfl_xor(da[b], o);
            }
        }
#pragma unroll
        for (int b = 0; b < kRows; ++b) {
            if (!ok[b]) continue;
            const float a = expf(e[b] - m) / D;
            const float de = a * (da[b] - c);
#pragma unroll
            for (int kv = 0; kv < KV; ++kv) {
                float out[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    out[v] = fmaf(de, qv[kv][v], a * gv[kv][v]);
                    dq[kv][v] = fmaf(de, xv[b][kv][v], dq[kv][v]);
                }
                if (d_x != nullptr && col[kv] < F) store_vec<VEC>(d_x + idx[b] * lddx + col[kv], out);
            }
        }
    }
    for (int o = LG; o < kWave; o <<= 1) {
#pragma unroll
        for (int kv = 0; kv < KV; ++kv)
#pragma unroll
            for (int v = 0; v < VEC; ++v) dq[kv][v] += __shfl_xor(dq[kv][v], o);
    }
    if (grp != 0) return;
    float* dst = it.k == 0 ? d_q + g * lddq : slot_dq + int64_t(it.beg / kChunk) * F;
#pragma unroll
    for (int kv = 0; kv < KV; ++kv)
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            if (col[kv] + v < F) dst[col[kv] + v] = dq[kv][v];
}

__global__ void __launch_bounds__(kBlock) attend_backward_merge_kernel(const int32_t* __restrict__ row_ptr, int64_t G, int64_t N,
                                                                       int F, float* __restrict__ d_q, int64_t lddq,
                                                                       const float* __restrict__ slot_dq)
{
    const Item it = find_item(row_ptr, G, N, G + blockIdx.x);
    if (it.g < 0 || it.k != 1) return;
    const int nch = (it.gend - it.gbeg + kChunk - 1) / kChunk;
    for (int f = threadIdx.x; f < F; f += kBlock) {
        float acc = d_q[int64_t(it.g) * lddq + f];
#pragma unroll 4
        for (int k = 1; k < nch; ++k) acc += slot_dq[((int64_t(it.gbeg) + int64_t(k) * kChunk) / kChunk) * F + f];
        d_q[int64_t(it.g) * lddq + f] = acc;
    }
}

// how a row of F floats is spread over a wave
struct RowShape {
    int vec, kv, lg;
};

inline RowShape row_shape(int64_t F, bool vec4)
{
    RowShape s;
    s.vec = vec4 ? 4 : 1;
    const int64_t nv = (F + s.vec - 1) / s.vec;      // lanes' worth of columns
    s.kv = 1;
    s.lg = 0;
    if (nv >= kWave) {
        s.lg = 6;
        while (int64_t(s.kv) * kWave < nv) s.kv <<= 1;
    } else {
        while ((int64_t(1) << s.lg) < nv) ++s.lg;
    }
    return s;
}

int check_attend(const char* fn, int64_t G, int64_t N, int64_t F)
{
    if (G < 0 || N < 0 || F < 0) {
        set_error("%s: negative size (G = %lld, N = %lld, F = %lld)", fn, (long long)G, (long long)N, (long long)F);
        return TFGX_ERR_INVALID_ARG;
    }
    if (G >= kInt32Max || N > kInt32Max) {
        set_error("%s: G and N must fit int32 (G = %lld, N = %lld)", fn, (long long)G, (long long)N);
        return TFGX_ERR_INVALID_ARG;
    }
    if (F > TFGX_SET2SET_MAX_FEATURES) {
        set_error("%s: F = %lld exceeds TFGX_SET2SET_MAX_FEATURES = %d", fn, (long long)F, TFGX_SET2SET_MAX_FEATURES);
        return TFGX_ERR_INVALID_ARG;
    }
    return TFGX_OK;
}

int check_ld(const char* fn, const char* name, int64_t ld, int64_t least)
{
    if (ld < least) {
        set_error("%s: %s is too small (%lld < %lld)", fn, name, (long long)ld, (long long)least);
        return TFGX_ERR_INVALID_ARG;
    }
    return TFGX_OK;
}

int check_null(const char* fn, const void* const* ptrs, const char* const* names, int n)
{
    for (int i = 0; i < n; ++i)
        if (ptrs[i] == nullptr) {
            set_error("%s: %s is null", fn, names[i]);
            return TFGX_ERR_INVALID_ARG;
        }
    return TFGX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// sequence LSTM
inline bool units_ok(int64_t U) { return U >= 16 && U <= TFGX_LSTM_MAX_UNITS && U % 16 == 0; }
inline size_t seq_lds_bytes(int64_t U, int rows, bool resident)
{
    return sizeof(float) * (size_t(rows) * size_t(5 * U) + (resident ? size_t(U) * size_t(4 * U) : 0));
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// saved: per (b, t) 5U floats at (b * T + t) * 5U — the activated gates i, f, g, o, then c_t; after all of them c0 [B, U]
template <int ROWS, bool RES, bool SAVE>
__global__ void __launch_bounds__(1024) lstm_sequence_forward_kernel(const float* __restrict__ P, int64_t ldp, int64_t B, int T,
                                                                     const float* __restrict__ R, int U,
                                                                     const float* __restrict__ h0, const float* __restrict__ c0,
                                                                     float* __restrict__ h_seq, float* __restrict__ h_last,
                                                                     float* __restrict__ c_last, float* __restrict__ saved)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int N4 = 4 * U, tid = threadIdx.x;
    float* hs = lds;                    // [ROWS][U]
    float* gs = hs + ROWS * U;          // [ROWS][4U]
    float* Rs = gs + ROWS * N4;         // [U][4U] (RES only)
    const int64_t b0 = int64_t(blockIdx.x) * ROWS;

    if constexpr (RES) {
        for (int idx = tid; idx < U * N4; idx += N4) Rs[idx] = R[idx];
    }
    for (int idx = tid; idx < ROWS * U; idx += N4) {
        const int64_t bb = b0 + idx / U;
        hs[idx] = (h0 != nullptr && bb < B) ? h0[bb * U + idx % U] : 0.0f;
    }
    float c[ROWS], hl[ROWS];
#pragma unroll
    for (int rb = 0; rb < ROWS; ++rb) {
        const int64_t bb = b0 + rb;
        c[rb] = (tid < U && c0 != nullptr && bb < B) ? c0[bb * U + tid] : 0.0f;
        hl[rb] = 0.0f;
        if (SAVE && tid < U && bb < B) saved[B * int64_t(T) * (5 * U) + bb * U + tid] = c[rb];
    }
    __syncthreads();

    const int gate = tid / U;
    const float* Rcol = (RES ? Rs : R) + tid;
    for (int t = 0; t < T; ++t) {
        float p[ROWS], acc[ROWS];
#pragma unroll
        for (int rb = 0; rb < ROWS; ++rb) {
            const int64_t bb = b0 + rb;
            p[rb] = bb < B ? P[(bb * T + t) * ldp + tid] : 0.0f;
            acc[rb] = 0.0f;
        }
        for (int k = 0; k < U; k += 4) {
            float rv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) rv[i] = Rcol[(k + i) * N4];
#pragma unroll
            for (int rb = 0; rb < ROWS; ++rb) {
                const float4 h4 = *reinterpret_cast<const float4*>(hs + rb * U + k);
                acc[rb] = fmaf(h4.x, rv[0], acc[rb]);
                acc[rb] = fmaf(h4.y, rv[1], acc[rb]);
                acc[rb] = fmaf(h4.z, rv[2], acc[rb]);
                acc[rb] = fmaf(h4.w, rv[3], acc[rb]);
            }
        }
#pragma unroll
        for (int rb = 0; rb < ROWS; ++rb) {
            const int64_t bb = b0 + rb;
            const float z = p[rb] + acc[rb];
            const float a = gate == 2 ? tanhf(z) : sigmoidf_(z);
            gs[rb * N4 + tid] = a;
            if (SAVE && bb < B) saved[(bb * T + t) * (5 * U) + tid] = a;
        }
        __syncthreads();        // the gates are complete, every thread has read h_{t-1}
        if (tid < U) {
#pragma unroll
            for (int rb = 0; rb < ROWS; ++rb) {
                const int64_t bb = b0 + rb;
                const float* gr = gs + rb * N4 + tid;
                const float cn = gr[U] * c[rb] + gr[0] * gr[2 * U];
                const float h = gr[3 * U] * tanhf(cn);
                c[rb] = cn;
                hl[rb] = h;
                hs[rb * U + tid] = h;
                if (bb < B) {
                    if (h_seq != nullptr) h_seq[(bb * T + t) * U + tid] = h;
                    if (SAVE) saved[(bb * T + t) * (5 * U) + 4 * U + tid] = cn;
                }
            }
        }
        __syncthreads();
    }
    if (tid < U) {
#pragma unroll
        for (int rb = 0; rb < ROWS; ++rb) {
            const int64_t bb = b0 + rb;
            if (bb < B) {
                if (h_last != nullptr) h_last[bb * U + tid] = hl[rb];
                if (c_last != nullptr) c_last[bb * U + tid] = c[rb];
            }
        }
    }
}

template <int ROWS, bool RES>
__global__ void __launch_bounds__(1024) lstm_sequence_backward_kernel(int64_t B, int T, int U, const float* __restrict__ R,
                                                                      const float* __restrict__ h0,
                                                                      const float* __restrict__ d_h_seq,
                                                                      const float* __restrict__ d_h_last,
                                                                      const float* __restrict__ d_c_last,
                                                                      const float* __restrict__ saved, float* __restrict__ d_gates,
                                                                      float* __restrict__ h_prev, float* __restrict__ d_h0,
                                                                      float* __restrict__ d_c0)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int N4 = 4 * U, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    float* dzs = lds;                   // [ROWS][4U]
    float* dhs = dzs + ROWS * N4;       // [ROWS][U]
    float* Rs = dhs + ROWS * U;         // [U][4U] (RES only)
    const int64_t b0 = int64_t(blockIdx.x) * ROWS;
    const float* c0s = saved + B * int64_t(T) * (5 * U);

    if constexpr (RES) {
        for (int idx = tid; idx < U * N4; idx += N4) Rs[idx] = R[idx];
    }
    float dc_next[ROWS];
#pragma unroll
    for (int rb = 0; rb < ROWS; ++rb) {
        const int64_t bb = b0 + rb;
        dc_next[rb] = (tid < U && d_c_last != nullptr && bb < B) ? d_c_last[bb * U + tid] : 0.0f;
        if (tid < U) dhs[rb * U + tid] = (d_h_last != nullptr && bb < B) ? d_h_last[bb * U + tid] : 0.0f;
    }
    __syncthreads();

    for (int t = T - 1; t >= 0; --t) {
        if (tid < U) {
#pragma unroll
            for (int rb = 0; rb < ROWS; ++rb) {
                const int64_t bb = b0 + rb;
                float dz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (bb < B) {
                    const int64_t bt = bb * T + t;
                    const float* s = saved + bt * (5 * U) + tid;
                    const float gi = s[0], gf = s[U], gg = s[2 * U], go = s[3 * U], ct = s[4 * U];
                    float cp, hp;
                    if (t > 0) {
                        const float* sp = s - 5 * U;
                        cp = sp[4 * U];
                        hp = sp[3 * U] * tanhf(cp);
                    } else {
                        cp = c0s[bb * U + tid];
                        hp = h0 != nullptr ? h0[bb * U + tid] : 0.0f;
                    }
                    const float dh = dhs[rb * U + tid] + (d_h_seq != nullptr ? d_h_seq[bt * U + tid] : 0.0f);
                    const float tc = tanhf(ct);
                    const float dc = dc_next[rb] + dh * go * (1.0f - tc * tc);
                    dz[0] = dc * gg * gi * (1.0f - gi);
                    dz[1] = dc * cp * gf * (1.0f - gf);
                    dz[2] = dc * gi * (1.0f - gg * gg);
                    dz[3] = dh * tc * go * (1.0f - go);
                    dc_next[rb] = dc * gf;
#pragma unroll
                    for (int g = 0; g < 4; ++g) d_gates[bt * N4 + g * U + tid] = dz[g];
                    h_prev[bt * U + tid] = hp;
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) dzs[rb * N4 + g * U + tid] = dz[g];
            }
        }
        __syncthreads();
        // dh_{t-1}[u] = <dz_t, R[u, :]>: wave w owns u = 16 w .. 16 w + 15 (U / 16 waves), lanes stride the 4U columns
        for (int uu = 0; uu < 16; ++uu) {
            const int u = wave * 16 + uu;
            const float* Rrow = (RES ? Rs : R) + int64_t(u) * N4;
            float part[ROWS];
#pragma unroll
            for (int rb = 0; rb < ROWS; ++rb) part[rb] = 0.0f;
            for (int j = lane; j < N4; j += kWave) {
                const float rv = Rrow[j];
#pragma unroll
                for (int rb = 0; rb < ROWS; ++rb) part[rb] = fmaf(dzs[rb * N4 + j], rv, part[rb]);
            }
#pragma unroll
            for (int o = kWave / 2; o > 0; o >>= 1)
#pragma unroll
                for (int rb = 0; rb < ROWS; ++rb) part[rb] += __shfl_xor(part[rb], o);
            if (lane == 0) {
#pragma unroll
                for (int rb = 0; rb < ROWS; ++rb) dhs[rb * U + u] = part[rb];
            }
        }
        __syncthreads();
    }
    if (tid < U) {
#pragma unroll
        for (int rb = 0; rb < ROWS; ++rb) {
            const int64_t bb = b0 + rb;
            if (bb < B) {
                d_h0[bb * U + tid] = dhs[rb * U + tid];
                d_c0[bb * U + tid] = dc_next[rb];
            }
        }
    }
}

int check_sequence(const char* fn, int64_t B, int64_t T, int64_t U)
{
    if (B < 0 || T < 0 || U < 0) {
        set_error("%s: negative size (B = %lld, T = %lld, U = %lld)", fn, (long long)B, (long long)T, (long long)U);
        return TFGX_ERR_INVALID_ARG;
    }
    if (U != 0 && !units_ok(U)) {
        set_error("%s: U must be a multiple of 16 in [16, %d], got %lld", fn, TFGX_LSTM_MAX_UNITS, (long long)U);
        return TFGX_ERR_INVALID_ARG;
    }
    if (B > kInt32Max || T > kInt32Max || (B > 0 && T > kInt32Max / B)) {
        set_error("%s: B * T must fit int32 (B = %lld, T = %lld)", fn, (long long)B, (long long)T);
        return TFGX_ERR_INVALID_ARG;
    }
    return TFGX_OK;
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_set2set_version(void) { return TFGX_SET2SET_ABI_VERSION; }

extern "C" size_t tfgx_set2set_attend_workspace_bytes(int64_t N, int64_t G, int64_t F)
{
    if (N <= kChunk || G <= 0 || F <= 0) return 0;
    return sizeof(float) * (size_t(2 * G) + size_t(slots_of(N)) * size_t(F + 2));
}

#define TFGX_ATTEND_DISPATCH(LAUNCH)                          \
    do {                                                      \
        if (shape.vec == 4) {                                 \
            if (shape.kv == 1) LAUNCH(4, 1);                  \
            else if (shape.kv == 2) LAUNCH(4, 2);             \
            else LAUNCH(4, 4);                                \
        } else {                                              \
            if (shape.kv == 1) LAUNCH(1, 1);                  \
            else if (shape.kv == 2) LAUNCH(1, 2);             \
            else if (shape.kv == 4) LAUNCH(1, 4);             \
            else if (shape.kv == 8) LAUNCH(1, 8);             \
            else LAUNCH(1, 16);                               \
        }                                                     \
    } while (0)

extern "C" int tfgx_set2set_attend_f32(const int32_t* row_ptr, const int32_t* node, int64_t G, int64_t N, const float* x, int64_t ldx,
                                       int64_t F, const float* q, int64_t ldq, float* r, int64_t ldr, float* stats, void* workspace,
                                       size_t workspace_bytes, int32_t* bad_flag, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_attend(__func__, G, N, F)) return rc;
    if (int rc = check_ld(__func__, "ldx", ldx, F)) return rc;
    if (int rc = check_ld(__func__, "ldq", ldq, F)) return rc;
    if (int rc = check_ld(__func__, "ldr", ldr, F)) return rc;
    if (G == 0 || F == 0) return TFGX_OK;
    {
        const void* ptrs[] = {row_ptr, q, r};
        const char* names[] = {"row_ptr", "q", "r"};
        if (int rc = check_null(__func__, ptrs, names, 3)) return rc;
    }
    if (N > 0) {
        const void* ptrs[] = {node, x};
        const char* names[] = {"node", "x"};
        if (int rc = check_null(__func__, ptrs, names, 2)) return rc;
    }
    const size_t need = tfgx_set2set_attend_workspace_bytes(N, G, F);
    if (need > 0 && workspace == nullptr) {
        set_error("%s: workspace is null (%zu bytes are needed)", __func__, need);
        return TFGX_ERR_INVALID_ARG;
    }
    if (workspace_bytes < need) {
        set_error("%s: workspace_bytes is too small (%zu < %zu)", __func__, workspace_bytes, need);
        return TFGX_ERR_INVALID_ARG;
    }
    const int64_t nslots = slots_of(N);
    const Workspace ws = carve(workspace, G, nslots);
    const RowShape shape = row_shape(F, F % 4 == 0 && ldx % 4 == 0 && aligned_to(x, 16));
    const int64_t blocks = (G + nslots + kWaves - 1) / kWaves;
#define TFGX_ATTEND_FWD(VEC_, KV_)                                                                                             \
    attend_forward_kernel<VEC_, KV_><<<dim3(unsigned(blocks)), kBlock, 0, stream>>>(row_ptr, node, G, N, nslots, x, ldx, int(F), \
                                                                                    shape.lg, q, ldq, r, ldr, stats, ws, bad_flag)
    TFGX_ATTEND_DISPATCH(TFGX_ATTEND_FWD);
#undef TFGX_ATTEND_FWD
    TFGX_LAUNCH_CHECK("attend_forward_kernel");
    if (nslots > 0) {
        attend_merge_kernel<<<dim3(unsigned(nslots)), kBlock, 0, stream>>>(row_ptr, G, N, int(F), r, ldr, stats, ws);
        TFGX_LAUNCH_CHECK("attend_merge_kernel");
    }
    return TFGX_OK;
}

extern "C" int tfgx_set2set_attend_backward_f32(const int32_t* row_ptr, const int32_t* node, int64_t G, int64_t N, const float* x,
                                                int64_t ldx, int64_t F, const float* q, int64_t ldq, const float* r, int64_t ldr,
                                                const float* stats, const float* d_r, int64_t ldg, float* d_x, int64_t lddx,
                                                float* d_q, int64_t lddq, void* workspace, size_t workspace_bytes,
                                                tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_attend(__func__, G, N, F)) return rc;
    if (int rc = check_ld(__func__, "ldx", ldx, F)) return rc;
    if (int rc = check_ld(__func__, "ldq", ldq, F)) return rc;
    if (int rc = check_ld(__func__, "ldr", ldr, F)) return rc;
    if (int rc = check_ld(__func__, "ldg", ldg, F)) return rc;
    if (d_x != nullptr)
        if (int rc = check_ld(__func__, "lddx", lddx, F)) return rc;
    if (int rc = check_ld(__func__, "lddq", lddq, F)) return rc;
    if (G == 0 || F == 0) return TFGX_OK;
    {
        const void* ptrs[] = {row_ptr, q, r, stats, d_r, d_q};
        const char* names[] = {"row_ptr", "q", "r", "stats", "d_r", "d_q"};
        if (int rc = check_null(__func__, ptrs, names, 6)) return rc;
    }
    if (N > 0) {
        const void* ptrs[] = {node, x};
        const char* names[] = {"node", "x"};
        if (int rc = check_null(__func__, ptrs, names, 2)) return rc;
    }
    const size_t need = tfgx_set2set_attend_workspace_bytes(N, G, F);
    if (need > 0 && workspace == nullptr) {
        set_error("%s: workspace is null (%zu bytes are needed)", __func__, need);
        return TFGX_ERR_INVALID_ARG;
    }
    if (workspace_bytes < need) {
        set_error("%s: workspace_bytes is too small (%zu < %zu)", __func__, workspace_bytes, need);
        return TFGX_ERR_INVALID_ARG;
    }
    const int64_t nslots = slots_of(N);
    float* slot_dq = carve(workspace, G, nslots).slot_r;
    const bool vec4 = F % 4 == 0 && ldx % 4 == 0 && aligned_to(x, 16) && (d_x == nullptr || (lddx % 4 == 0 && aligned_to(d_x, 16)));
    const RowShape shape = row_shape(F, vec4);
    const int64_t blocks = (G + nslots + kWaves - 1) / kWaves;
#define TFGX_ATTEND_BWD(VEC_, KV_)                                                                                              \
    attend_backward_kernel<VEC_, KV_><<<dim3(unsigned(blocks)), kBlock, 0, stream>>>(row_ptr, node, G, N, nslots, x, ldx, int(F), \
                                                                                     shape.lg, q, ldq, r, ldr, stats, d_r, ldg,  \
                                                                                     d_x, lddx, d_q, lddq, slot_dq)
    TFGX_ATTEND_DISPATCH(TFGX_ATTEND_BWD);
#undef TFGX_ATTEND_BWD
    TFGX_LAUNCH_CHECK("attend_backward_kernel");
    if (nslots > 0) {
        attend_backward_merge_kernel<<<dim3(unsigned(nslots)), kBlock, 0, stream>>>(row_ptr, G, N, int(F), d_q, lddq, slot_dq);
        TFGX_LAUNCH_CHECK("attend_backward_merge_kernel");
    }
    return TFGX_OK;
}

extern "C" int tfgx_lstm_sequence_kernel_resident(int64_t U)
{
    if (!units_ok(U)) return 0;
    return seq_lds_bytes(U, 4, true) <= kLdsLimit ? 1 : 0;
}

extern "C" size_t tfgx_lstm_sequence_saved_bytes(int64_t B, int64_t T, int64_t U)
{
    if (B <= 0 || T <= 0 || U <= 0) return 0;
    return sizeof(float) * size_t(B) * size_t(U) * (5 * size_t(T) + 1);
}

// the kernels may use up to kLdsLimit of dynamic LDS: raised once per instantiation
template <typename K>
int allow_big_lds(K kernel, bool& done)
{
    if (!done) {
        TFGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           int(kLdsLimit)));
        done = true;
    }
    return TFGX_OK;
}

extern "C" int tfgx_lstm_sequence_f32(const float* P, int64_t ldp, int64_t B, int64_t T, const float* R, int64_t U, const float* h0,
                                      const float* c0, float* h_seq, float* h_last, float* c_last, void* saved, size_t saved_bytes,
                                      tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_sequence(__func__, B, T, U)) return rc;
    if (int rc = check_ld(__func__, "ldp", ldp, 4 * U)) return rc;
    if (B == 0 || T == 0 || U == 0) return TFGX_OK;
    {
        const void* ptrs[] = {P, R};
        const char* names[] = {"P", "R"};
        if (int rc = check_null(__func__, ptrs, names, 2)) return rc;
    }
    if (saved != nullptr && saved_bytes < tfgx_lstm_sequence_saved_bytes(B, T, U)) {
        set_error("%s: saved_bytes is too small (%zu < %zu)", __func__, saved_bytes, tfgx_lstm_sequence_saved_bytes(B, T, U));
        return TFGX_ERR_INVALID_ARG;
    }
    const bool res = tfgx_lstm_sequence_kernel_resident(U) != 0 && T >= 2;
    const int rows = B == 1 ? 1 : 4;
    const size_t lds_bytes = seq_lds_bytes(U, rows, res);
    const unsigned grid = unsigned((B + rows - 1) / rows), block = unsigned(4 * U);
#define TFGX_SEQ_FWD(ROWS_, RES_, SAVE_)                                                                                    \
    do {                                                                                                                    \
        static bool attr_set = false;                                                                                       \
        if (int rc = allow_big_lds(lstm_sequence_forward_kernel<ROWS_, RES_, SAVE_>, attr_set)) return rc;                  \
        lstm_sequence_forward_kernel<ROWS_, RES_, SAVE_><<<grid, block, lds_bytes, stream>>>(                               \
            P, ldp, B, int(T), R, int(U), h0, c0, h_seq, h_last, c_last, static_cast<float*>(saved));                       \
    } while (0)
#define TFGX_SEQ_FWD_ROWS(ROWS_)                                   \
    do {                                                           \
        if (res && saved != nullptr) TFGX_SEQ_FWD(ROWS_, true, true);   \
        else if (res) TFGX_SEQ_FWD(ROWS_, true, false);            \
        else if (saved != nullptr) TFGX_SEQ_FWD(ROWS_, false, true);    \
        else TFGX_SEQ_FWD(ROWS_, false, false);                    \
    } while (0)
    if (rows == 1) TFGX_SEQ_FWD_ROWS(1);
    else TFGX_SEQ_FWD_ROWS(4);
#undef TFGX_SEQ_FWD_ROWS
#undef TFGX_SEQ_FWD
    TFGX_LAUNCH_CHECK("lstm_sequence_forward_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_lstm_sequence_backward_f32(int64_t B, int64_t T, int64_t U, const float* R, const float* h0, const float* d_h_seq,
                                               const float* d_h_last, const float* d_c_last, const void* saved, size_t saved_bytes,
                                               float* d_gates, float* h_prev, float* d_h0, float* d_c0, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_sequence(__func__, B, T, U)) return rc;
    if (B == 0 || T == 0 || U == 0) return TFGX_OK;
    {
        const void* ptrs[] = {R, saved, d_gates, h_prev, d_h0, d_c0};
        const char* names[] = {"R", "saved", "d_gates", "h_prev", "d_h0", "d_c0"};
        if (int rc = check_null(__func__, ptrs, names, 6)) return rc;
    }
    if (saved_bytes < tfgx_lstm_sequence_saved_bytes(B, T, U)) {
        set_error("%s: saved_bytes is too small (%zu < %zu)", __func__, saved_bytes, tfgx_lstm_sequence_saved_bytes(B, T, U));
        return TFGX_ERR_INVALID_ARG;
    }
    const bool res = tfgx_lstm_sequence_kernel_resident(U) != 0 && T >= 2;
    const int rows = B == 1 ? 1 : 4;
    const size_t lds_bytes = seq_lds_bytes(U, rows, res);
    const unsigned grid = unsigned((B + rows - 1) / rows), block = unsigned(4 * U);
#define TFGX_SEQ_BWD(ROWS_, RES_)                                                                                           \
    do {                                                                                                                    \
        static bool attr_set = false;                                                                                       \
        if (int rc = allow_big_lds(lstm_sequence_backward_kernel<ROWS_, RES_>, attr_set)) return rc;                        \
        lstm_sequence_backward_kernel<ROWS_, RES_><<<grid, block, lds_bytes, stream>>>(                                     \
            B, int(T), int(U), R, h0, d_h_seq, d_h_last, d_c_last, static_cast<const float*>(saved), d_gates, h_prev, d_h0, d_c0); \
    } while (0)
    if (rows == 1 && res) TFGX_SEQ_BWD(1, true);
    else if (rows == 1) TFGX_SEQ_BWD(1, false);
    else if (res) TFGX_SEQ_BWD(4, true);
    else TFGX_SEQ_BWD(4, false);
#undef TFGX_SEQ_BWD
    TFGX_LAUNCH_CHECK("lstm_sequence_backward_kernel");
    return TFGX_OK;
}
