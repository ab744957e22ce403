// ASAP pooling's two hot paths (include/tfgx_asap.h): the fused 1-hop attention with the one launch its backward needs, and
// the sparse S^T A S of cluster_pool by expand - sort - compress.
//
// Reference: nn/pool/asap.py:67-85 and nn/pool/cluster_pool.py:32-38, nn/kernel/segment.py:26-33.
//
// Attention.  The forward kernel lives in tfgx_asap_attend.h (shared with tfgx_asap_static.hip): a wave per destination row,
// 64 edges at a time, the running (m, l, acc) carried.  The backward kernel is below.
//
// S^T A S.  count: valid entries per row of S, products per edge, an int64 exclusive scan (hipcub), the total to the host.
// emit: a thread per edge writes its products at offsets[e] + i * deg(v) + j.  reduce: hipcub's stable radix sort on the
// 64-bit keys, a thread per run head sums its run in order, an exclusive scan of the keep flags places the survivors, and
// the row pointer is read off the compacted rows.
#include "tfgx_common.h"
#include "tfgx_host.h"
#include "tfgx_asap_attend.h"
#include "../../include/tfgx_asap.h"
#include <hipcub/hipcub.hpp>

namespace tfgx {
namespace {

using asap_attend::kWaves;
using asap_attend::kAlpha;
using asap_attend::wave_sum;
constexpr int64_t kInt32Max = (int64_t(1) << 31) - 1;

// attention backward (the weights): see the header
__global__ void __launch_bounds__(kBlock) asap_attend_backward_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                      int64_t N, int64_t E, const float* __restrict__ sq,
                                                                      const float* __restrict__ sh, const float* __restrict__ bias,
                                                                      const float* __restrict__ p, const float* __restrict__ p_self,
                                                                      const float* __restrict__ pd, const float* __restrict__ pd_self,
                                                                      const float* __restrict__ dp, const float* __restrict__ dp_self,
                                                                      float* __restrict__ ds, float* __restrict__ ds_self,
                                                                      float* __restrict__ dsq)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const float b0 = *bias;
    for (int64_t row = int64_t(blockIdx.x) * kWaves + wave; row < N; row += int64_t(gridDim.x) * kWaves) {
        int64_t beg = row_ptr[row], end = row_ptr[row + 1];
        if (!(beg >= 0 && end >= beg && end <= E)) beg = end = 0;
        const float sqr = sq[row] + b0;
        float t = 0.0f;
        for (int64_t i = beg + lane; i < end; i += kWave) t += pd[i] * dp[i];
        const float self_term = pd_self[row] * dp_self[row];
        t = wave_sum(t) + self_term;
        float acc = 0.0f;
        for (int64_t i = beg + lane; i < end; i += kWave) {
            const int32_t cj = col[i];
            const bool ok = cj >= 0 && int64_t(cj) < N;
            float v = 0.0f;
            if (ok) {
                const float z = sqr + sh[cj];
                v = (pd[i] * dp[i] - p[i] * t) * (z > 0.0f ? 1.0f : kAlpha);
            }
            ds[i] = v;
            acc += v;
        }
        acc = wave_sum(acc);
        if (lane == 0) {
            const float z = sqr + sh[row];
            const float v = (self_term - p_self[row] * t) * (z > 0.0f ? 1.0f : kAlpha);
            ds_self[row] = v;
            dsq[row] = acc + v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// S^T A S

__global__ void spasp_row_degree(const int32_t* __restrict__ s_row_ptr, const int32_t* __restrict__ s_col, int64_t N, int32_t K,
                                 int32_t* __restrict__ s_deg)
{
    int64_t u = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; u < N; u += stride) {
        int32_t d = 0;
        for (int32_t i = s_row_ptr[u]; i < s_row_ptr[u + 1]; ++i) {
            const int32_t cl = s_col[i];
            d += (cl >= 0 && cl < K) ? 1 : 0;
        }
        s_deg[u] = d;
    }
}

__global__ void spasp_edge_count(const int32_t* __restrict__ a_row, const int32_t* __restrict__ a_col, int64_t E, int64_t N,
                                 const int32_t* __restrict__ s_deg, int64_t* __restrict__ cnt, int32_t* __restrict__ bad)
{
    int64_t e = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    int any_bad = 0;
    for (; e <= E; e += stride) {
        int64_t v = 0;
        if (e < E) {
            const int32_t u = a_row[e], w = a_col[e];
            if (u < 0 || u >= N || w < 0 || w >= N) any_bad = 1;
            else v = int64_t(s_deg[u]) * int64_t(s_deg[w]);
        }
        cnt[e] = v;      // cnt[E] = 0: the exclusive scan leaves the total there
    }
    if (__any(any_bad) && (threadIdx.x & 63) == 0) atomicOr(bad, 1);
}

__global__ void spasp_emit_kernel(const int32_t* __restrict__ s_row_ptr, const int32_t* __restrict__ s_col,
                                  const float* __restrict__ s_val, int64_t N, int32_t K, const int32_t* __restrict__ a_row,
                                  const int32_t* __restrict__ a_col, const float* __restrict__ a_val, int64_t E,
                                  const int32_t* __restrict__ s_deg, const int64_t* __restrict__ offsets, int64_t total,
                                  uint64_t* __restrict__ keys, float* __restrict__ vals)
{
    int64_t e = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; e < E; e += stride) {
        const int32_t u = a_row[e], v = a_col[e];
        if (u < 0 || u >= N || v < 0 || v >= N) continue;      // count refused such a list; never an out-of-range read
        const int64_t base = offsets[e];
        const int64_t dv = s_deg[v];
        const int64_t n_out = offsets[e + 1] - base;
        if (n_out != int64_t(s_deg[u]) * dv || base < 0 || base + n_out > total) continue;      // offsets of another graph
        const float a = a_val != nullptr ? a_val[e] : 1.0f;
        int64_t i = 0;
        for (int32_t iu = s_row_ptr[u]; iu < s_row_ptr[u + 1]; ++iu) {
            const int32_t c1 = s_col[iu];
            if (c1 < 0 || c1 >= K) continue;
            if (i >= int64_t(s_deg[u])) break;
            const float sa = (s_val != nullptr ? s_val[iu] : 1.0f) * a;
            int64_t j = 0;
            for (int32_t iv = s_row_ptr[v]; iv < s_row_ptr[v + 1]; ++iv) {
                const int32_t c2 = s_col[iv];
                if (c2 < 0 || c2 >= K) continue;
                if (j >= dv) break;
                const int64_t o = base + i * dv + j;
                keys[o] = (uint64_t(uint32_t(c1)) << 32) | uint32_t(c2);
                vals[o] = sa * (s_val != nullptr ? s_val[iv] : 1.0f);
                ++j;
            }
            ++i;
        }
    }
}

// a thread per run head: the run's sum in sorted order, and whether the entry stays
__global__ void spasp_run_sums(const uint64_t* __restrict__ keys_s, const float* __restrict__ vals_s, int64_t total,
                               int32_t drop_diagonal, float* __restrict__ sums, int32_t* __restrict__ keep)
{
    int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; i < total; i += stride) {
        const uint64_t key = keys_s[i];
        int32_t k = 0;
        if (i == 0 || keys_s[i - 1] != key) {
            float s = vals_s[i];
            for (int64_t j = i + 1; j < total && keys_s[j] == key; ++j) s += vals_s[j];
            sums[i] = s;
            k = (s != 0.0f) && !(drop_diagonal && uint32_t(key >> 32) == uint32_t(key));
        }
        keep[i] = k;
    }
}

__global__ void spasp_compact(const uint64_t* __restrict__ keys_s, const float* __restrict__ sums, const int32_t* __restrict__ keep,
                              const int32_t* __restrict__ place, int64_t total, int32_t* __restrict__ out_row,
                              int32_t* __restrict__ out_col, float* __restrict__ out_val, int32_t* __restrict__ out_count)
{
    int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; i < total; i += stride) {
        if (keep[i]) {
            const int32_t o = place[i];
            const uint64_t key = keys_s[i];
            out_row[o] = int32_t(key >> 32);
            out_col[o] = int32_t(uint32_t(key));
            out_val[o] = sums[i];
        }
        if (i == total - 1) *out_count = place[i] + keep[i];
    }
}

// row_ptr[r] = the first output position whose row is >= r, for r in [0, K]
__global__ void spasp_row_ptr(const int32_t* __restrict__ out_row, const int32_t* __restrict__ out_count, int32_t K,
                              int32_t* __restrict__ row_ptr)
{
    const int64_t n = *out_count;
    int64_t o = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; o <= n; o += stride) {
        int32_t lo = (o == 0) ? 0 : out_row[o - 1] + 1;
        int32_t hi = (o == n) ? K : out_row[o];
        if (lo < 0) lo = 0;
        if (hi > K) hi = K;
        for (int32_t r = lo; r <= hi; ++r) row_ptr[r] = int32_t(o);
    }
}

struct CountLayout {
    size_t cnt, bad, temp, total;
};

CountLayout count_layout(int64_t E)
{
    size_t t = 0;
    const int64_t* in = nullptr;
    int64_t* out = nullptr;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t, in, out, static_cast<int>(E + 1));
    CountLayout L;
    size_t o = 0;
    L.cnt = o, o += align256(8 * size_t(E + 1));
    L.bad = o, o += 256;
    L.temp = o, o += align256(t) + 256;
    L.total = o;
    return L;
}

struct SpaspLayout {
    size_t keys, keys_s, vals, vals_s, keep, place, temp, total;
};

SpaspLayout spasp_layout(int64_t total)
{
    const size_t n = size_t(total);
    size_t t1 = 0, t2 = 0;
    const uint64_t* k = nullptr;
    uint64_t* ko = nullptr;
    const float* v = nullptr;
    float* vo = nullptr;
    const int32_t* f = nullptr;
    int32_t* fo = nullptr;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t1, k, ko, v, vo, static_cast<int>(n), 0, 64);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t2, f, fo, static_cast<int>(n));
    SpaspLayout L;
    size_t o = 0;
    L.keys = o, o += align256(8 * n);
    L.keys_s = o, o += align256(8 * n);
    L.vals = o, o += align256(4 * n);      // the products; after the sort, the run sums
    L.vals_s = o, o += align256(4 * n);
    L.keep = o, o += align256(4 * n);
    L.place = o, o += align256(4 * n);
    L.temp = o, o += align256(t1 > t2 ? t1 : t2) + 256;
    L.total = o;
    return L;
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_asap_version(void) { return TFGX_ASAP_ABI_VERSION; }

extern "C" int tfgx_asap_attend_f32(const int32_t* row_ptr, const int32_t* col, int64_t N, int64_t E, const float* x,
                                    int64_t ldx, int64_t F, const float* sq, const float* sh, const float* bias,
                                    float drop_rate, uint64_t seed, float* c, int64_t ldc, float* p, float* p_self,
                                    float* p_drop, float* p_self_drop, int32_t* bad_flag, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    TFGX_REQUIRE(N >= 0 && E >= 0 && F >= 0, "negative size");
    TFGX_REQUIRE(N + E <= kInt32Max, "N + E must fit int32");
    TFGX_REQUIRE(F <= TFGX_ASAP_MAX_FEATURES, "F exceeds TFGX_ASAP_MAX_FEATURES");
    TFGX_REQUIRE(ldx >= F, "ldx < F");
    TFGX_REQUIRE(ldc >= F, "ldc < F");
    TFGX_REQUIRE(drop_rate >= 0.0f && drop_rate < 1.0f, "drop_rate must be in [0, 1)");
    if (N == 0) return TFGX_OK;
    TFGX_REQUIRE(row_ptr != nullptr, "row_ptr is null");
    TFGX_REQUIRE(col != nullptr || E == 0, "col is null");
    TFGX_REQUIRE(x != nullptr || F == 0, "x is null");
    TFGX_REQUIRE(c != nullptr || F == 0, "c is null");
    TFGX_REQUIRE(sq != nullptr, "sq is null");
    TFGX_REQUIRE(sh != nullptr, "sh is null");
    TFGX_REQUIRE(bias != nullptr, "bias is null");
    TFGX_REQUIRE(p != nullptr || E == 0, "p is null");
    TFGX_REQUIRE(p_self != nullptr, "p_self is null");
    if (drop_rate > 0.0f) {
        TFGX_REQUIRE(p_drop != nullptr || E == 0, "p_drop is null (required with drop_rate > 0)");
        TFGX_REQUIRE(p_self_drop != nullptr, "p_self_drop is null (required with drop_rate > 0)");
    }
    hipStream_t stream = as_stream(stream_);
    const DropCfg drop = make_drop(drop_rate, seed, E);
    asap_attend::launch<false>(row_ptr, col, N, E, x, ldx, F, sq, sh, bias, drop, c, ldc, p, p_self, p_drop, p_self_drop, bad_flag,
                               stream);
    TFGX_LAUNCH_CHECK("asap_attend_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_asap_attend_backward_f32(const int32_t* row_ptr, const int32_t* col, int64_t N, int64_t E, const float* sq,
                                             const float* sh, const float* bias, const float* p, const float* p_self,
                                             const float* p_drop, const float* p_self_drop, const float* dp,
                                             const float* dp_self, float* ds, float* ds_self, float* dsq, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    TFGX_REQUIRE(N >= 0 && E >= 0, "negative size");
    TFGX_REQUIRE(N + E <= kInt32Max, "N + E must fit int32");
    if (N == 0) return TFGX_OK;
    TFGX_REQUIRE(row_ptr != nullptr, "row_ptr is null");
    TFGX_REQUIRE(col != nullptr || E == 0, "col is null");
    TFGX_REQUIRE(sq != nullptr, "sq is null");
    TFGX_REQUIRE(sh != nullptr, "sh is null");
    TFGX_REQUIRE(bias != nullptr, "bias is null");
    TFGX_REQUIRE(p != nullptr || E == 0, "p is null");
    TFGX_REQUIRE(p_self != nullptr, "p_self is null");
    TFGX_REQUIRE((p_drop == nullptr) == (p_self_drop == nullptr) || E == 0, "give both p_drop and p_self_drop, or neither");
    TFGX_REQUIRE(dp != nullptr || E == 0, "dp is null");
    TFGX_REQUIRE(dp_self != nullptr, "dp_self is null");
    TFGX_REQUIRE(ds != nullptr || E == 0, "ds is null");
    TFGX_REQUIRE(ds_self != nullptr, "ds_self is null");
    TFGX_REQUIRE(dsq != nullptr, "dsq is null");
    hipStream_t stream = as_stream(stream_);
    asap_attend_backward_kernel<<<grid_for(N, kWaves), kBlock, 0, stream>>>(
        row_ptr, col, N, E, sq, sh, bias, p, p_self, p_drop != nullptr ? p_drop : p,
        p_self_drop != nullptr ? p_self_drop : p_self, dp, dp_self, ds, ds_self, dsq);
    TFGX_LAUNCH_CHECK("asap_attend_backward_kernel");
    return TFGX_OK;
}

extern "C" size_t tfgx_spasp_count_workspace_bytes(int64_t N, int64_t E)
{
    if (N < 0 || E < 0 || E >= kInt32Max) return 0;
    return count_layout(E).total;
}

extern "C" size_t tfgx_spasp_workspace_bytes(int64_t total, int64_t K)
{
    if (total <= 0 || total > kInt32Max || K <= 0 || K > kInt32Max) return 0;
    return spasp_layout(total).total;
}

extern "C" int tfgx_spasp_count(const int32_t* s_row_ptr, const int32_t* s_col, int64_t N, int64_t K, const int32_t* a_row,
                                const int32_t* a_col, int64_t E, int32_t* s_deg, int64_t* offsets, int64_t* total,
                                void* workspace, size_t workspace_bytes, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    TFGX_REQUIRE(N >= 0 && K >= 0 && E >= 0, "negative size");
    TFGX_REQUIRE(N <= kInt32Max && K <= kInt32Max && E < kInt32Max, "sizes must fit int32");
    TFGX_REQUIRE(total != nullptr, "total is null");
    TFGX_REQUIRE(offsets != nullptr, "offsets is null");
    hipStream_t stream = as_stream(stream_);
    *total = 0;
    if (N == 0 || K == 0 || E == 0) {
        TFGX_HIP_CHECK(hipMemsetAsync(offsets, 0, sizeof(int64_t) * size_t(E + 1), stream));
        if (N > 0 && s_deg != nullptr) TFGX_HIP_CHECK(hipMemsetAsync(s_deg, 0, sizeof(int32_t) * size_t(N), stream));
        return TFGX_OK;
    }
    TFGX_REQUIRE(s_row_ptr != nullptr, "s_row_ptr is null");
    TFGX_REQUIRE(s_col != nullptr, "s_col is null");
    TFGX_REQUIRE(a_row != nullptr, "a_row is null");
    TFGX_REQUIRE(a_col != nullptr, "a_col is null");
    TFGX_REQUIRE(s_deg != nullptr, "s_deg is null");
    TFGX_REQUIRE(workspace != nullptr, "workspace is null");
    const CountLayout lay = count_layout(E);
    if (workspace_bytes < lay.total) {
        set_error("tfgx_spasp_count: workspace_bytes too small (%zu < %zu)", workspace_bytes, lay.total);
        return TFGX_ERR_WORKSPACE;
    }
    char* ws = static_cast<char*>(workspace);
    int64_t* cnt = reinterpret_cast<int64_t*>(ws + lay.cnt);
    int32_t* bad = reinterpret_cast<int32_t*>(ws + lay.bad);
    TFGX_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), stream));
    spasp_row_degree<<<grid_for(N, kBlock), kBlock, 0, stream>>>(s_row_ptr, s_col, N, int32_t(K), s_deg);
    TFGX_LAUNCH_CHECK("spasp_row_degree");
    spasp_edge_count<<<grid_for(E + 1, kBlock), kBlock, 0, stream>>>(a_row, a_col, E, N, s_deg, cnt, bad);
    TFGX_LAUNCH_CHECK("spasp_edge_count");
    size_t tb = workspace_bytes - lay.temp;
    TFGX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(ws + lay.temp, tb, cnt, offsets, static_cast<int>(E + 1), stream));
    int64_t total_host = 0;
    int32_t bad_host = 0;
    TFGX_HIP_CHECK(hipMemcpyAsync(&total_host, offsets + E, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    TFGX_HIP_CHECK(hipMemcpyAsync(&bad_host, bad, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    TFGX_HIP_CHECK(hipStreamSynchronize(stream));
    if (bad_host) {
        set_error("tfgx_spasp_count: an edge endpoint is outside [0, %lld)", (long long)N);
        return TFGX_ERR_INDEX;
    }
    *total = total_host;
    if (total_host > kInt32Max) {
        set_error("tfgx_spasp_count: the expansion has %lld products, above 2^31 - 1", (long long)total_host);
        return TFGX_ERR_INVALID_ARG;
    }
    return TFGX_OK;
}

extern "C" int tfgx_spasp_emit(const int32_t* s_row_ptr, const int32_t* s_col, const float* s_val, int64_t N, int64_t K,
                               const int32_t* a_row, const int32_t* a_col, const float* a_val, int64_t E, const int32_t* s_deg,
                               const int64_t* offsets, int64_t total, void* workspace, size_t workspace_bytes,
                               tfgx_stream_t stream_)
{
    TFGX_RANGE();
    TFGX_REQUIRE(N >= 0 && K >= 0 && E >= 0 && total >= 0, "negative size");
    TFGX_REQUIRE(total <= kInt32Max, "total exceeds 2^31 - 1");
    TFGX_REQUIRE(N <= kInt32Max && K <= kInt32Max && E < kInt32Max, "sizes must fit int32");
    if (total == 0 || E == 0) return TFGX_OK;
    TFGX_REQUIRE(K > 0 && N > 0, "total > 0 with an empty S");
    TFGX_REQUIRE(s_row_ptr != nullptr, "s_row_ptr is null");
    TFGX_REQUIRE(s_col != nullptr, "s_col is null");
    TFGX_REQUIRE(a_row != nullptr, "a_row is null");
    TFGX_REQUIRE(a_col != nullptr, "a_col is null");
    TFGX_REQUIRE(s_deg != nullptr, "s_deg is null");
    TFGX_REQUIRE(offsets != nullptr, "offsets is null");
    TFGX_REQUIRE(workspace != nullptr, "workspace is null");
    const SpaspLayout lay = spasp_layout(total);
    if (workspace_bytes < lay.total) {
        set_error("tfgx_spasp_emit: workspace_bytes too small (%zu < %zu)", workspace_bytes, lay.total);
        return TFGX_ERR_WORKSPACE;
    }
    hipStream_t stream = as_stream(stream_);
    char* ws = static_cast<char*>(workspace);
    uint64_t* keys = reinterpret_cast<uint64_t*>(ws + lay.keys);
    float* vals = reinterpret_cast<float*>(ws + lay.vals);
    // a position no edge writes (offsets that do not belong to these inputs) must not reach the sort uninitialised
    TFGX_HIP_CHECK(hipMemsetAsync(keys, 0xFF, sizeof(uint64_t) * size_t(total), stream));
    TFGX_HIP_CHECK(hipMemsetAsync(vals, 0, sizeof(float) * size_t(total), stream));
    spasp_emit_kernel<<<grid_for(E, kBlock), kBlock, 0, stream>>>(s_row_ptr, s_col, s_val, N, int32_t(K), a_row, a_col, a_val, E,
                                                                   s_deg, offsets, total, keys, vals);
    TFGX_LAUNCH_CHECK("spasp_emit_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_spasp_reduce(int64_t total, int64_t K, int32_t drop_diagonal, int32_t* out_row, int32_t* out_col,
                                 float* out_val, int32_t* out_row_ptr, int32_t* out_count, void* workspace,
                                 size_t workspace_bytes, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    TFGX_REQUIRE(total >= 0 && K >= 0, "negative size");
    TFGX_REQUIRE(total <= kInt32Max, "total exceeds 2^31 - 1");
    TFGX_REQUIRE(K < kInt32Max, "K must fit int32");
    TFGX_REQUIRE(out_count != nullptr, "out_count is null");
    TFGX_REQUIRE(out_row_ptr != nullptr, "out_row_ptr is null");
    hipStream_t stream = as_stream(stream_);
    if (total == 0 || K == 0) {
        TFGX_HIP_CHECK(hipMemsetAsync(out_count, 0, sizeof(int32_t), stream));
        TFGX_HIP_CHECK(hipMemsetAsync(out_row_ptr, 0, sizeof(int32_t) * size_t(K + 1), stream));
        return TFGX_OK;
    }
    TFGX_REQUIRE(out_row != nullptr, "out_row is null");
    TFGX_REQUIRE(out_col != nullptr, "out_col is null");
    TFGX_REQUIRE(out_val != nullptr, "out_val is null");
    TFGX_REQUIRE(workspace != nullptr, "workspace is null");
    const SpaspLayout lay = spasp_layout(total);
    if (workspace_bytes < lay.total) {
        set_error("tfgx_spasp_reduce: workspace_bytes too small (%zu < %zu)", workspace_bytes, lay.total);
        return TFGX_ERR_WORKSPACE;
    }
    char* ws = static_cast<char*>(workspace);
    uint64_t* keys = reinterpret_cast<uint64_t*>(ws + lay.keys);
    uint64_t* keys_s = reinterpret_cast<uint64_t*>(ws + lay.keys_s);
    float* vals = reinterpret_cast<float*>(ws + lay.vals);
    float* vals_s = reinterpret_cast<float*>(ws + lay.vals_s);
    int32_t* keep = reinterpret_cast<int32_t*>(ws + lay.keep);
    int32_t* place = reinterpret_cast<int32_t*>(ws + lay.place);
    void* temp = ws + lay.temp;
    const size_t temp_bytes = workspace_bytes - lay.temp;
    const int n = static_cast<int>(total);
    size_t tb = temp_bytes;
    // keys of positions emit did not write are all ones: the sort needs every bit of them to keep them last
    TFGX_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp, tb, keys, keys_s, vals, vals_s, n, 0, 64, stream));
    float* sums = vals;      // the unsorted products are not needed any more
    spasp_run_sums<<<grid_for(total, kBlock), kBlock, 0, stream>>>(keys_s, vals_s, total, drop_diagonal, sums, keep);
    TFGX_LAUNCH_CHECK("spasp_run_sums");
    tb = temp_bytes;
    TFGX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(temp, tb, keep, place, n, stream));
    spasp_compact<<<grid_for(total, kBlock), kBlock, 0, stream>>>(keys_s, sums, keep, place, total, out_row, out_col, out_val,
                                                                   out_count);
    TFGX_LAUNCH_CHECK("spasp_compact");
    spasp_row_ptr<<<grid_for(total + 1, kBlock), kBlock, 0, stream>>>(out_row, out_count, int32_t(K), out_row_ptr);
    TFGX_LAUNCH_CHECK("spasp_row_ptr");
    return TFGX_OK;
}
