// The segmented transposed product out[g] = S_g^T Y_g of the dense pooling layers and its backward (include/tfgx_seggram.h).
//
// Reference: nn/pool/diff_pool.py:42-48, nn/pool/min_cut_pool.py:31-89 (a sparse [N, G K] assignment against a dense [N, N]
// adjacency; here the block structure is used instead: [K, n_g] x [n_g, W] per graph, ragged in n_g).
//
// Forward.  The position axis is cut at the absolute multiples of kB.  A workgroup stages the S rows and 64 columns of the Y
// rows of its block in LDS (coalesced row pieces; the rows are gathered through seg_node), then walks the segments that meet
// the block in order.  Thread (wave q, lane c) owns column c and the KPT clusters q KPT .. q KPT + KPT - 1 of the accumulator
// tile: one fma chain per element over the positions of the run, S read as a wave-wide broadcast and Y conflict-free.  A run
// that is the whole segment goes to out, any other to the workspace: slot 0 of the block when the segment came in from the
// block before, slot 1 when it starts here and leaves.  The fold adds a crossing segment's partials in block order, in two
// levels so that one long segment is not one long chain: groups of kF partials first (seggram_group_kernel, a workgroup per
// group), then per segment (a workgroup per segment and 1024 output elements) the first partial, the groups and the
// partials left over; that launch also writes the zero rows of empty segments and reports bad spans.
//
// Backward.  A workgroup takes kR consecutive nodes, splits them into runs of equal segment id, and per 64 columns of W keeps
// the run's dOut block in LDS (rows padded to 65 floats: the dS threads read a column of it).  dY rows are written per tile,
// dS is carried in registers over the tiles: up to 8 (node, cluster) pairs per thread.
#include "tfgx_common.h"
#include "../../include/tfgx_seggram.h"

namespace tfgx {
namespace {

constexpr int kB = 64;                       // positions per block
constexpr int kWT = 64;                      // columns of W per workgroup
constexpr int kKG = kBlock / kWT;            // cluster groups (waves) per workgroup
constexpr int kFoldPerBlock = 4 * kBlock;    // output elements per fold workgroup
constexpr int kF = 64;                       // partials per group of the two-level fold
constexpr int kR = 32;                       // nodes per backward workgroup
constexpr int kPairs = kR * TFGX_SEGGRAM_MAX_K / kBlock;      // (node, cluster) pairs per backward thread
constexpr int kDoLd = kWT + 1;
constexpr int64_t kInt32Max = (int64_t(1) << 31) - 1;
constexpr int kGridCap = 1 << 20;
constexpr int64_t kMaxW = int64_t(1) << 20;    // keeps grid.y of both forward launches below 65536

__device__ __forceinline__ bool span_ok(int64_t beg, int64_t end, int64_t N) { return beg >= 0 && beg <= end && end <= N; }

template <int KPT>
__global__ void __launch_bounds__(kBlock) seggram_fwd_kernel(const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ seg_node,
                                                             int64_t G, int64_t N, int64_t nblocks,
                                                             const float* __restrict__ S, int64_t lds, int K,
                                                             const float* __restrict__ Y, int64_t ldy, int64_t W,
                                                             float* __restrict__ out, int64_t ldo, float* __restrict__ ws,
                                                             int32_t* __restrict__ flag)
{
    extern __shared__ float smem[];
    float* Ss = smem;                         // [kB, K]
    float* Ys = smem + kB * K;                // [kB, kWT]
    int* nodes = reinterpret_cast<int*>(Ys + kB * kWT);      // [kB], then the first segment of the block
    const int tid = threadIdx.x, c = tid & (kWT - 1), kbase = (tid / kWT) * KPT;
    const int64_t w0 = int64_t(blockIdx.y) * kWT;
    const int wt = int(W - w0 < kWT ? W - w0 : kWT);
    int bad = 0;
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const int64_t p0 = b * kB, p1 = (p0 + kB < N) ? p0 + kB : N;
        const int nb = int(p1 - p0);
        for (int i = tid; i < nb; i += kBlock) {
            int64_t n = seg_node ? int64_t(seg_node[p0 + i]) : p0 + i;
            if (n < 0 || n >= N) { n = -1; bad = 1; }
            nodes[i] = int(n);
        }
        if (tid == 0) {          // the first segment whose end lies beyond the block's first position
            int64_t lo = 0, hi = G;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (int64_t(seg_ptr[mid + 1]) > p0) hi = mid; else lo = mid + 1;
            }
            nodes[kB] = int(lo);
        }
        __syncthreads();
        for (int i = tid; i < nb * K; i += kBlock) {
            const int r = i / K, k = i - r * K, n = nodes[r];
            Ss[i] = n >= 0 ? S[int64_t(n) * lds + k] : 0.0f;
        }
        for (int i = tid; i < nb * kWT; i += kBlock) {
            const int r = i / kWT, cc = i & (kWT - 1), n = nodes[r];
            Ys[i] = (n >= 0 && cc < wt) ? Y[int64_t(n) * ldy + w0 + cc] : 0.0f;
        }
        __syncthreads();
        for (int64_t g = nodes[kB]; g < G; ++g) {
            const int64_t beg = seg_ptr[g], end = seg_ptr[g + 1];
            if (!span_ok(beg, end, N)) continue;          // reported by the fold launch
            if (beg >= p1) break;
            const int lo = int((beg > p0 ? beg : p0) - p0), hi = int((end < p1 ? end : p1) - p0);
            if (hi > lo) {
                float acc[KPT];
#pragma unroll
                for (int i = 0; i < KPT; ++i) acc[i] = 0.0f;
                for (int p = lo; p < hi; ++p) {
                    const float y = Ys[p * kWT + c];
                    const float* s = Ss + p * K + kbase;
#pragma unroll
                    for (int i = 0; i < KPT; ++i)
                        if (kbase + i < K) acc[i] = fmaf(s[i], y, acc[i]);
                }
                float* dst;
                int64_t ld;
                if (beg >= p0 && end <= p1) {
                    dst = out + g * K * ldo + w0;
                    ld = ldo;
                } else {
                    dst = ws + (b * 2 + (beg < p0 ? 0 : 1)) * K * W + w0;
                    ld = W;
                }
                if (c < wt) {
#pragma unroll
                    for (int i = 0; i < KPT; ++i)
                        if (kbase + i < K) dst[(kbase + i) * ld + c] = acc[i];
                }
            }
            if (end > p1) break;
        }
        __syncthreads();
    }
    if (bad && flag && blockIdx.y == 0) atomicOr(flag, 1);
}

__global__ void __launch_bounds__(kBlock) seggram_fold_kernel(const int32_t* __restrict__ seg_ptr, int64_t G, int64_t N, int K,
                                                              int64_t W, float* __restrict__ out, int64_t ldo,
                                                              const float* __restrict__ ws, int32_t* __restrict__ flag)
{
    const int64_t KW = int64_t(K) * W;
    const int64_t e0 = int64_t(blockIdx.y) * kFoldPerBlock + threadIdx.x;
    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const int64_t beg = seg_ptr[g], end = seg_ptr[g + 1];
        const bool ok = span_ok(beg, end, N);
        if (!ok && flag && threadIdx.x == 0 && blockIdx.y == 0) atomicOr(flag, 1);
        const bool empty = !ok || end == beg;
        const int64_t b0 = empty ? 0 : beg / kB, b1 = empty ? 0 : (end - 1) / kB;
        if (!empty && b0 == b1) continue;                 // written by its block
#pragma unroll
        for (int j = 0; j < kFoldPerBlock / kBlock; ++j) {
            const int64_t e = e0 + int64_t(j) * kBlock;
            if (e >= KW) break;
            float acc = 0.0f;
            if (!empty) {
                acc = ws[(b0 * 2 + 1) * KW + e];
                const int64_t groups = (b1 - b0) / kF;          // folded by seggram_group_kernel into slot 1 of their first block
#pragma unroll 4
                for (int64_t q = 0; q < groups; ++q) acc += ws[((b0 + 1 + q * kF) * 2 + 1) * KW + e];
#pragma unroll 8
                for (int64_t b = b0 + 1 + groups * kF; b <= b1; ++b) acc += ws[b * 2 * KW + e];
            }
            const int64_t k = e / W;
            out[(g * K + k) * ldo + (e - k * W)] = acc;
        }
    }
}

// The first level of the fold.  The blocks b0 + 1 .. b1 of a segment that crosses boundaries each hold one incoming partial
// (slot 0); they are taken kF at a time, counted from the segment's OWN first block, and every full group is added up in block
// order into slot 1 of the group's first block, which nothing else uses: that block lies wholly inside the segment, and slot 1
// belongs to a segment that starts in its block.  A workgroup per block decides for itself whether its block opens a group.
__global__ void __launch_bounds__(kBlock) seggram_group_kernel(const int32_t* __restrict__ seg_ptr, int64_t G, int64_t N,
                                                               int64_t nblocks, int K, int64_t W, float* ws)
{
    __shared__ int opens;
    const int64_t KW = int64_t(K) * W;
    const int64_t e0 = int64_t(blockIdx.y) * kFoldPerBlock + threadIdx.x;
    for (int64_t b = int64_t(blockIdx.x) + 1; b + kF - 1 < nblocks; b += gridDim.x) {
        if (threadIdx.x == 0) {
            const int64_t p = b * kB;
            int64_t lo = 0, hi = G;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (int64_t(seg_ptr[mid + 1]) > p) hi = mid; else lo = mid + 1;
            }
            int ok = 0;
            if (lo < G) {
                const int64_t beg = seg_ptr[lo], end = seg_ptr[lo + 1];
                if (span_ok(beg, end, N) && beg < p && end > p) {
                    const int64_t b0 = beg / kB, b1 = (end - 1) / kB;
                    ok = (b - b0 - 1) % kF == 0 && b + kF - 1 <= b1;
                }
            }
            opens = ok;
        }
        __syncthreads();
        const bool go = opens != 0;
        __syncthreads();
        if (!go) continue;
#pragma unroll
        for (int j = 0; j < kFoldPerBlock / kBlock; ++j) {
            const int64_t e = e0 + int64_t(j) * kBlock;
            if (e >= KW) break;
            float acc = ws[b * 2 * KW + e];
#pragma unroll 8
            for (int i = 1; i < kF; ++i) acc += ws[(b + i) * 2 * KW + e];
            ws[(b * 2 + 1) * KW + e] = acc;
        }
    }
}

template <bool WANT_DS, bool WANT_DY>
__global__ void __launch_bounds__(kBlock) seggram_bwd_kernel(const int32_t* __restrict__ node_seg, int64_t N, int64_t G,
                                                             const float* __restrict__ S, int64_t lds, int K,
                                                             const float* __restrict__ Y, int64_t ldy, int64_t W,
                                                             const float* __restrict__ dOut, int64_t ldo,
                                                             float* __restrict__ dS, int64_t ldds, float* __restrict__ dY,
                                                             int64_t lddy, int32_t* __restrict__ flag)
{
    __shared__ float Ss[kR * TFGX_SEGGRAM_MAX_K];
    __shared__ float Ys[kR * kWT];
    __shared__ float dOs[TFGX_SEGGRAM_MAX_K * kDoLd];
    __shared__ int segs[kR];
    const int tid = threadIdx.x, c = tid & (kWT - 1), q = tid / kWT;
    const int64_t runs = (N + kR - 1) / kR;
    int bad = 0;
    for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
        const int64_t n0 = run * kR;
        const int nr = int(N - n0 < kR ? N - n0 : kR);
        if (tid < nr) {
            int64_t g = node_seg[n0 + tid];
            if (g < 0 || g >= G) { g = -1; bad = 1; }
            segs[tid] = int(g);
        }
        if (WANT_DY)
            for (int i = tid; i < nr * K; i += kBlock) {
                const int r = i / K, k = i - r * K;
                Ss[i] = S[(n0 + r) * lds + k];
            }
        float accS[kPairs];
#pragma unroll
        for (int j = 0; j < kPairs; ++j) accS[j] = 0.0f;
        __syncthreads();
        for (int64_t w0 = 0; w0 < W; w0 += kWT) {
            const int wt = int(W - w0 < kWT ? W - w0 : kWT);
            if (WANT_DS)
                for (int i = tid; i < nr * kWT; i += kBlock) {
                    const int r = i / kWT, cc = i & (kWT - 1);
                    Ys[i] = cc < wt ? Y[(n0 + r) * ldy + w0 + cc] : 0.0f;
                }
            for (int lo = 0; lo < nr;) {
                const int g = segs[lo];
                int hi = lo + 1;
                while (hi < nr && segs[hi] == g) ++hi;
                for (int i = tid; i < K * kWT; i += kBlock) {
                    const int k = i / kWT, cc = i & (kWT - 1);
                    dOs[k * kDoLd + cc] = (g >= 0 && cc < wt) ? dOut[(int64_t(g) * K + k) * ldo + w0 + cc] : 0.0f;
                }
                __syncthreads();
                if (WANT_DY)
                    for (int r = lo + q; r < hi; r += kBlock / kWT) {
                        float a = 0.0f;
                        for (int k = 0; k < K; ++k) a = fmaf(Ss[r * K + k], dOs[k * kDoLd + c], a);
                        if (c < wt) dY[(n0 + r) * lddy + w0 + c] = a;
                    }
                if (WANT_DS) {
#pragma unroll
                    for (int j = 0; j < kPairs; ++j) {
                        const int i = tid + j * kBlock;
                        const int r = i / K, k = i - r * K;
                        if (r >= lo && r < hi) {
                            float a = accS[j];
                            for (int cc = 0; cc < kWT; ++cc) a = fmaf(Ys[r * kWT + cc], dOs[k * kDoLd + cc], a);
                            accS[j] = a;
                        }
                    }
                }
                __syncthreads();
                lo = hi;
            }
        }
        if (WANT_DS) {
#pragma unroll
            for (int j = 0; j < kPairs; ++j) {
                const int i = tid + j * kBlock;
                const int r = i / K, k = i - r * K;
                if (r < nr) dS[(n0 + r) * ldds + k] = accS[j];
            }
        }
        __syncthreads();
    }
    if (bad && flag) atomicOr(flag, 1);
}

int64_t blocks_of(int64_t N) { return (N + kB - 1) / kB; }

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_seggram_version(void) { return TFGX_SEGGRAM_ABI_VERSION; }

extern "C" int tfgx_seggram_block(void) { return kB; }

extern "C" size_t tfgx_segment_gram_workspace_bytes(int64_t N, int64_t G, int64_t K, int64_t W)
{
    if (N < 0 || G <= 0 || K < 1 || K > TFGX_SEGGRAM_MAX_K || W <= 0 || N > kInt32Max) return 0;
    const int64_t nb = blocks_of(N);
    if (nb <= 1) return 0;          // no segment can cross a boundary
    return size_t(nb) * 2 * size_t(K) * size_t(W) * sizeof(float);
}

extern "C" int tfgx_segment_gram_f32(const int32_t* seg_ptr, const int32_t* seg_node, int64_t G, int64_t N, const float* S,
                                     int64_t lds, int64_t K, const float* Y, int64_t ldy, int64_t W, float* out, int64_t ldo,
                                     int32_t* bad_flag, void* workspace, size_t workspace_bytes, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    TFGX_REQUIRE(N >= 0 && G >= 0 && W >= 0, "negative size");
    TFGX_REQUIRE(K >= 1 && K <= TFGX_SEGGRAM_MAX_K, "K must be in [1, TFGX_SEGGRAM_MAX_K]");
    TFGX_REQUIRE(N <= kInt32Max && G * K <= kInt32Max, "N and G * K must fit int32");
    TFGX_REQUIRE(W <= kMaxW, "W exceeds 2^20");
    TFGX_REQUIRE(lds >= K, "lds < K");
    TFGX_REQUIRE(ldy >= W, "ldy < W");
    TFGX_REQUIRE(ldo >= W, "ldo < W");
    if (G == 0 || W == 0) return TFGX_OK;
    TFGX_REQUIRE(seg_ptr != nullptr, "seg_ptr is null");
    TFGX_REQUIRE(out != nullptr, "out is null");
    TFGX_REQUIRE(S != nullptr || N == 0, "S is null");
    TFGX_REQUIRE(Y != nullptr || N == 0, "Y is null");
    const size_t need = tfgx_segment_gram_workspace_bytes(N, G, K, W);
    TFGX_REQUIRE(workspace != nullptr || need == 0, "workspace is null");
    if (workspace_bytes < need) {
        set_error("tfgx_segment_gram_f32: workspace_bytes too small (%zu < %zu)", workspace_bytes, need);
        return TFGX_ERR_WORKSPACE;
    }
    hipStream_t stream = as_stream(stream_);
    const int k = int(K);
    const int64_t nb = blocks_of(N);
    float* ws = static_cast<float*>(workspace);
    if (nb > 0) {
        const dim3 grid(unsigned(nb < kGridCap ? nb : kGridCap), unsigned((W + kWT - 1) / kWT));
        const size_t smem = (size_t(kB) * k + size_t(kB) * kWT) * sizeof(float) + (kB + 1) * sizeof(int);
#define TFGX_SEGGRAM_LAUNCH(KPT)                                                                                                  \
    seggram_fwd_kernel<KPT><<<grid, kBlock, smem, stream>>>(seg_ptr, seg_node, G, N, nb, S, lds, k, Y, ldy, W, out, ldo, ws,     \
                                                            bad_flag)
        if (k <= kKG) TFGX_SEGGRAM_LAUNCH(1);
        else if (k <= 2 * kKG) TFGX_SEGGRAM_LAUNCH(2);
        else if (k <= 4 * kKG) TFGX_SEGGRAM_LAUNCH(4);
        else if (k <= 8 * kKG) TFGX_SEGGRAM_LAUNCH(8);
        else TFGX_SEGGRAM_LAUNCH(16);
#undef TFGX_SEGGRAM_LAUNCH
        TFGX_LAUNCH_CHECK("seggram_fwd_kernel");
    }
    const unsigned tiles = unsigned((K * W + kFoldPerBlock - 1) / kFoldPerBlock);
    if (nb > kF) {          // a segment can hold a full group of partials
        const dim3 ggrid(unsigned(nb - kF < kGridCap ? nb - kF : kGridCap), tiles);
        seggram_group_kernel<<<ggrid, kBlock, 0, stream>>>(seg_ptr, G, N, nb, k, W, ws);
        TFGX_LAUNCH_CHECK("seggram_group_kernel");
    }
    const dim3 fgrid(unsigned(G < kGridCap ? G : kGridCap), tiles);
    seggram_fold_kernel<<<fgrid, kBlock, 0, stream>>>(seg_ptr, G, N, k, W, out, ldo, ws, bad_flag);
    TFGX_LAUNCH_CHECK("seggram_fold_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_segment_gram_backward_f32(const int32_t* node_seg, int64_t N, int64_t G, const float* S, int64_t lds,
                                              int64_t K, const float* Y, int64_t ldy, int64_t W, const float* dOut, int64_t ldo,
                                              float* dS, int64_t ldds, float* dY, int64_t lddy, int32_t* bad_flag,
                                              tfgx_stream_t stream_)
{
    TFGX_RANGE();
    TFGX_REQUIRE(N >= 0 && G >= 0 && W >= 0, "negative size");
    TFGX_REQUIRE(K >= 1 && K <= TFGX_SEGGRAM_MAX_K, "K must be in [1, TFGX_SEGGRAM_MAX_K]");
    TFGX_REQUIRE(N <= kInt32Max && G * K <= kInt32Max, "N and G * K must fit int32");
    TFGX_REQUIRE(W <= kMaxW, "W exceeds 2^20");
    TFGX_REQUIRE(ldo >= W, "ldo < W");
    TFGX_REQUIRE(dS == nullptr || ldds >= K, "ldds < K");
    TFGX_REQUIRE(dY == nullptr || lddy >= W, "lddy < W");
    TFGX_REQUIRE(dS == nullptr || ldy >= W, "ldy < W");
    TFGX_REQUIRE(dY == nullptr || lds >= K, "lds < K");
    if (N == 0 || (dS == nullptr && (dY == nullptr || W == 0))) return TFGX_OK;
    TFGX_REQUIRE(node_seg != nullptr, "node_seg is null");
    TFGX_REQUIRE(dOut != nullptr || W == 0 || G == 0, "dOut is null");
    TFGX_REQUIRE(dS == nullptr || Y != nullptr || W == 0, "Y is null");
    TFGX_REQUIRE(dY == nullptr || S != nullptr, "S is null");
    hipStream_t stream = as_stream(stream_);
    const int64_t runs = (N + kR - 1) / kR;
    const int grid = int(runs < kGridCap ? runs : kGridCap);
    const int k = int(K);
    if (dS && dY)
        seggram_bwd_kernel<true, true><<<grid, kBlock, 0, stream>>>(node_seg, N, G, S, lds, k, Y, ldy, W, dOut, ldo, dS, ldds, dY,
                                                                    lddy, bad_flag);
    else if (dS)
        seggram_bwd_kernel<true, false><<<grid, kBlock, 0, stream>>>(node_seg, N, G, S, lds, k, Y, ldy, W, dOut, ldo, dS, ldds, dY,
                                                                     lddy, bad_flag);
    else
        seggram_bwd_kernel<false, true><<<grid, kBlock, 0, stream>>>(node_seg, N, G, S, lds, k, Y, ldy, W, dOut, ldo, dS, ldds, dY,
                                                                     lddy, bad_flag);
    TFGX_LAUNCH_CHECK("seggram_bwd_kernel");
    return TFGX_OK;
}
