// Link prediction (include/tfgx_linkpred.h): the per-edge dot-product decoder and the rejection samplers.
//
// Reference: demo/demo_gae.py (logit = reduce_sum(gather(z, row) * gather(z, col))), utils/graph_utils.py:369-452.
//
// edge_dot: two random row gathers per edge over an unsorted list — the traffic of one aggregation pass with no plan.
// wave64; a 16-lane group owns kEdgesPerGroup = 4 consecutive edges at a time, so a wave holds 16 edges = 32 row
// gathers in flight.  Per 64-column chunk every lane issues all 8 of its loads (a and b piece of 4 edges) before the
// first product.  Nothing in the chunk loop is predicated: edge ids past E, endpoints out of range and columns past F
// are CLAMPED to a valid address and their contribution is zeroed by a select afterwards (a load under a
// branch makes the compiler drain every outstanding gather).  The 16 partial sums meet in a fixed xor tree.
//
// Samplers: one thread per slot; attempts 0, 1, ... of negative_draw until the candidate passes the filter (a binary
// search inside one row of the sorted adjacency).  Plain stores; integer atomics on the caller's counter word only.
#include "tfgx_common.h"
#include "../../include/tfgx_linkpred.h"

namespace tfgx {
namespace {

constexpr int kGroup = 16;                                   // lanes per edge
constexpr int kEdgesPerGroup = 4;                            // edges a group gathers together
constexpr int kGroupsPerBlock = kBlock / kGroup;
constexpr int kEdgesPerBlock = kGroupsPerBlock * kEdgesPerGroup;      // 64
constexpr int kChunk = 64;                                   // columns per chunk (16 lanes x 4 floats)
constexpr int64_t kMaxNodes = (int64_t(1) << 31) - 1;

// VEC = 4: lane l reads the float4 at column 64 k + 4 l.  VEC = 1: lane l reads columns 64 k + 16 t + l, t = 0 .. 3.
template <int VEC>
__global__ void __launch_bounds__(kBlock) edge_dot_kernel(const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                          int64_t E, const float* __restrict__ a, int64_t lda, int64_t n_a,
                                                          const float* __restrict__ b, int64_t ldb, int64_t n_b, int F,
                                                          float* __restrict__ out, int32_t* __restrict__ flag)
{
    const int lane = threadIdx.x & (kGroup - 1), grp = threadIdx.x / kGroup;
    const int64_t n_batches = (E + kEdgesPerBlock - 1) / kEdgesPerBlock;
    const int n_chunks = (F + kChunk - 1) / kChunk;
    int bad = 0;
    for (int64_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
        const int64_t e0 = batch * kEdgesPerBlock + int64_t(grp) * kEdgesPerGroup;
        const float* pa[kEdgesPerGroup];
        const float* pb[kEdgesPerGroup];
        bool ok[kEdgesPerGroup];
#pragma unroll
        for (int u = 0; u < kEdgesPerGroup; ++u) {
            const int64_t e = e0 + u < E ? e0 + u : E - 1;              // E >= 1 here: a valid edge for the padded slots
            const int32_t r = row[e], c = col[e];
            ok[u] = (r >= 0) & (int64_t(r) < n_a) & (c >= 0) & (int64_t(c) < n_b);
            bad |= !ok[u];
            pa[u] = a + int64_t(ok[u] ? r : 0) * lda;                   // n_a, n_b >= 1 here: row 0 exists
            pb[u] = b + int64_t(ok[u] ? c : 0) * ldb;
        }
        float acc[kEdgesPerGroup];
#pragma unroll
        for (int u = 0; u < kEdgesPerGroup; ++u) acc[u] = 0.0f;
        for (int k = 0; k < n_chunks; ++k) {
            if constexpr (VEC == 4) {
                const int j = k * kChunk + 4 * lane;
                const bool valid = j < F;                               // F % 4 == 0: the whole float4 is inside
                const int jo = valid ? j : 0;
                float4 av[kEdgesPerGroup], bv[kEdgesPerGroup];
#pragma unroll
                for (int u = 0; u < kEdgesPerGroup; ++u) {
                    av[u] = *reinterpret_cast<const float4*>(pa[u] + jo);
                    bv[u] = *reinterpret_cast<const float4*>(pb[u] + jo);
                }
#pragma unroll
                for (int u = 0; u < kEdgesPerGroup; ++u) {
                    float t = acc[u];
                    t = fmaf(av[u].x, bv[u].x, t);
                    t = fmaf(av[u].y, bv[u].y, t);
                    t = fmaf(av[u].z, bv[u].z, t);
                    t = fmaf(av[u].w, bv[u].w, t);
                    acc[u] = valid ? t : acc[u];
                }
            } else {
                float av[kEdgesPerGroup][4], bv[kEdgesPerGroup][4];
                bool valid[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int j = k * kChunk + kGroup * t + lane;
                    valid[t] = j < F;
                    const int jo = valid[t] ? j : 0;
#pragma unroll
                    for (int u = 0; u < kEdgesPerGroup; ++u) {
                        av[u][t] = pa[u][jo];
                        bv[u][t] = pb[u][jo];
                    }
                }
#pragma unroll
                for (int u = 0; u < kEdgesPerGroup; ++u)
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[u] = valid[t] ? fmaf(av[u][t], bv[u][t], acc[u]) : acc[u];
            }
        }
#pragma unroll
        for (int u = 0; u < kEdgesPerGroup; ++u) {
#pragma unroll
            for (int o = kGroup / 2; o > 0; o >>= 1) acc[u] += __shfl_xor(acc[u], o, kGroup);
            acc[u] = ok[u] ? acc[u] : 0.0f;
        }
        // every lane holds the four sums: lane u stores edge e0 + u (one 16-byte run per group)
        float mine = acc[0];
#pragma unroll
        for (int u = 1; u < kEdgesPerGroup; ++u) mine = lane == u ? acc[u] : mine;
        if (lane < kEdgesPerGroup && e0 + lane < E) out[e0 + lane] = mine;
    }
    if (flag != nullptr && __any(bad) && (threadIdx.x & (kWave - 1)) == 0) atomicOr(flag, 1);
}

__global__ void raise_flag(int32_t* flag) { atomicOr(flag, 1); }

// ---- the draw (tfgx_negative_draw restates it on the host)
__host__ __device__ inline uint64_t slot_key(uint64_t seed, uint64_t slot)
{
    const uint32_t hi = drop_hash(seed, uint32_t(slot));
    const uint32_t lo = drop_hash(seed ^ 0x9E3779B97F4A7C15ull, uint32_t(slot >> 32) ^ hi);
    return (uint64_t(hi) << 32) | lo;
}

__host__ __device__ inline void draw_pair(uint64_t key, uint32_t attempt, uint64_t n, int32_t& u, int32_t& v)
{
    u = int32_t((uint64_t(drop_hash(key, 2u * attempt)) * n) >> 32);
    v = int32_t((uint64_t(drop_hash(key, 2u * attempt + 1u)) * n) >> 32);
}

// is c in the strictly ascending adj_col[adj_ptr[r] .. adj_ptr[r + 1])?
__device__ __forceinline__ bool has_edge(const int32_t* __restrict__ adj_ptr, const int32_t* __restrict__ adj_col, int32_t r,
                                         int32_t c)
{
    int32_t lo = adj_ptr[r], hi = adj_ptr[r + 1];
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        const int32_t x = adj_col[mid];
        if (x == c) return true;
        if (x < c) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

__global__ void __launch_bounds__(kBlock) sample_pairs_kernel(int64_t num_samples, uint64_t n, const int32_t* __restrict__ adj_ptr,
                                                              const int32_t* __restrict__ adj_col, int undirected, uint64_t seed,
                                                              uint64_t slot_base, int max_attempts, int32_t* __restrict__ out_row,
                                                              int32_t* __restrict__ out_col, int32_t* __restrict__ n_failed)
{
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t s = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; s < num_samples; s += stride) {
        const uint64_t key = slot_key(seed, slot_base + uint64_t(s));
        int32_t r = -1, c = -1;
        if (adj_ptr == nullptr) {
            draw_pair(key, 0u, n, r, c);
        } else {
            for (int t = 0; t < max_attempts; ++t) {
                int32_t u, v;
                draw_pair(key, uint32_t(t), n, u, v);
                if (u == v) continue;
                if (undirected && u > v) {
                    const int32_t w = u;
                    u = v;
                    v = w;
                }
                if (has_edge(adj_ptr, adj_col, u, v)) continue;
                r = u;
                c = v;
                break;
            }
            if (r < 0) atomicAdd(n_failed, 1);
        }
        out_row[s] = r;
        out_col[s] = c;
    }
}

__global__ void __launch_bounds__(kBlock) sample_from_kernel(const int32_t* __restrict__ start, int64_t num_samples, uint64_t n,
                                                             const int32_t* __restrict__ adj_ptr, const int32_t* __restrict__ adj_col,
                                                             uint64_t seed, uint64_t slot_base, int max_attempts,
                                                             int32_t* __restrict__ out_col, int32_t* __restrict__ n_failed)
{
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t s = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; s < num_samples; s += stride) {
        const uint64_t key = slot_key(seed, slot_base + uint64_t(s));
        const int32_t a = start[s];
        int32_t c = -1;
        if (a < 0 || uint64_t(a) >= n) {
            atomicOr(n_failed, TFGX_NEGATIVE_BAD_START);
        } else if (adj_ptr == nullptr) {
            int32_t u;
            draw_pair(key, 0u, n, u, c);
        } else {
            for (int t = 0; t < max_attempts; ++t) {
                int32_t u, v;
                draw_pair(key, uint32_t(t), n, u, v);
                if (v == a || has_edge(adj_ptr, adj_col, a, v)) continue;
                c = v;
                break;
            }
            if (c < 0) atomicAdd(n_failed, 1);
        }
        out_col[s] = c;
    }
}

int check_sampler(const char* fn, int64_t num_samples, int64_t num_nodes, const int32_t* adj_ptr, const int32_t* adj_col,
                  int32_t max_attempts, const int32_t* n_failed)
{
    if (num_samples < 0) {
        set_error("%s: num_samples is negative (%lld)", fn, (long long)num_samples);
        return TFGX_ERR_INVALID_ARG;
    }
    if (num_nodes < 1 || num_nodes > kMaxNodes) {
        set_error("%s: num_nodes must be in [1, 2^31), got %lld", fn, (long long)num_nodes);
        return TFGX_ERR_INVALID_ARG;
    }
    if (max_attempts < 1) {
        set_error("%s: max_attempts must be at least 1, got %d", fn, int(max_attempts));
        return TFGX_ERR_INVALID_ARG;
    }
    if ((adj_ptr == nullptr) != (adj_col == nullptr)) {
        // an adjacency without entries still has a row_ptr; its col array may be any non-null pointer
        set_error("%s: %s is null but %s is not", fn, adj_ptr == nullptr ? "adj_ptr" : "adj_col",
                  adj_ptr == nullptr ? "adj_col" : "adj_ptr");
        return TFGX_ERR_INVALID_ARG;
    }
    if (n_failed == nullptr) {
        set_error("%s: n_failed is null", fn);
        return TFGX_ERR_INVALID_ARG;
    }
    return TFGX_OK;
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_linkpred_version(void) { return TFGX_LINKPRED_ABI_VERSION; }

extern "C" int tfgx_edge_dot_f32(const int32_t* row, const int32_t* col, int64_t E, const float* a, int64_t lda, int64_t n_a,
                                 const float* b, int64_t ldb, int64_t n_b, int64_t F, float* out, int32_t* bad_flag,
                                 tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (E < 0 || n_a < 0 || n_b < 0 || F < 0) {
        set_error("%s: negative size (E = %lld, n_a = %lld, n_b = %lld, F = %lld)", __func__, (long long)E, (long long)n_a,
                  (long long)n_b, (long long)F);
        return TFGX_ERR_INVALID_ARG;
    }
    if (n_a > kMaxNodes || n_b > kMaxNodes || F > kMaxNodes) {
        set_error("%s: n_a, n_b and F must fit int32", __func__);
        return TFGX_ERR_INVALID_ARG;
    }
    if (lda < F || ldb < F) {
        set_error("%s: %s is smaller than F (%lld < %lld)", __func__, lda < F ? "lda" : "ldb", (long long)(lda < F ? lda : ldb),
                  (long long)F);
        return TFGX_ERR_INVALID_ARG;
    }
    if (E == 0) return TFGX_OK;
    if (row == nullptr || col == nullptr || out == nullptr) {
        set_error("%s: %s is null", __func__, row == nullptr ? "row" : (col == nullptr ? "col" : "out"));
        return TFGX_ERR_INVALID_ARG;
    }
    if (n_a == 0 || n_b == 0) {          // every endpoint is out of range: zeros and the flag, no table is touched
        TFGX_HIP_CHECK(hipMemsetAsync(out, 0, sizeof(float) * size_t(E), stream));
        if (bad_flag != nullptr) {
            raise_flag<<<1, 1, 0, stream>>>(bad_flag);
            TFGX_LAUNCH_CHECK("raise_flag");
        }
        return TFGX_OK;
    }
    if (F == 0) {
        // an empty sum; endpoints are still validated by the kernel below (no column is read: n_chunks == 0)
    } else if (a == nullptr || b == nullptr) {
        set_error("%s: %s is null", __func__, a == nullptr ? "a" : "b");
        return TFGX_ERR_INVALID_ARG;
    }
    const int64_t n_batches = (E + kEdgesPerBlock - 1) / kEdgesPerBlock;
    const int grid = grid_for(n_batches, 1, kMaxGrid * 4);
    const bool vec4 = aligned_to(a, 16) && aligned_to(b, 16) && lda % 4 == 0 && ldb % 4 == 0 && F % 4 == 0;
    if (vec4)
        edge_dot_kernel<4><<<grid, kBlock, 0, stream>>>(row, col, E, a, lda, n_a, b, ldb, n_b, int(F), out, bad_flag);
    else
        edge_dot_kernel<1><<<grid, kBlock, 0, stream>>>(row, col, E, a, lda, n_a, b, ldb, n_b, int(F), out, bad_flag);
    TFGX_LAUNCH_CHECK("edge_dot_kernel");
    return TFGX_OK;
}

extern "C" void tfgx_negative_draw(uint64_t seed, uint64_t slot, uint32_t attempt, int64_t num_nodes, int32_t* u, int32_t* v)
{
    int32_t du = -1, dv = -1;
    if (num_nodes >= 1 && num_nodes <= kMaxNodes && attempt < (1u << 31))
        draw_pair(slot_key(seed, slot), attempt, uint64_t(num_nodes), du, dv);
    if (u != nullptr) *u = du;
    if (v != nullptr) *v = dv;
}

extern "C" int tfgx_negative_sample_pairs(int64_t num_samples, int64_t num_nodes, const int32_t* adj_ptr, const int32_t* adj_col,
                                          int32_t undirected, uint64_t seed, uint64_t slot_base, int32_t max_attempts,
                                          int32_t* out_row, int32_t* out_col, int32_t* n_failed, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_sampler(__func__, num_samples, num_nodes, adj_ptr, adj_col, max_attempts, n_failed)) return rc;
    TFGX_REQUIRE(undirected == 0 || undirected == 1, "undirected must be 0 or 1");
    if (num_samples == 0) return TFGX_OK;
    if (out_row == nullptr || out_col == nullptr) {
        set_error("%s: %s is null", __func__, out_row == nullptr ? "out_row" : "out_col");
        return TFGX_ERR_INVALID_ARG;
    }
    sample_pairs_kernel<<<grid_for(num_samples, kBlock), kBlock, 0, stream>>>(num_samples, uint64_t(num_nodes), adj_ptr, adj_col,
                                                                              undirected, seed, slot_base, max_attempts, out_row,
                                                                              out_col, n_failed);
    TFGX_LAUNCH_CHECK("sample_pairs_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_negative_sample_from(const int32_t* start, int64_t num_samples, int64_t num_nodes, const int32_t* adj_ptr,
                                         const int32_t* adj_col, uint64_t seed, uint64_t slot_base, int32_t max_attempts,
                                         int32_t* out_col, int32_t* n_failed, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_sampler(__func__, num_samples, num_nodes, adj_ptr, adj_col, max_attempts, n_failed)) return rc;
    if (num_samples == 0) return TFGX_OK;
    if (start == nullptr || out_col == nullptr) {
        set_error("%s: %s is null", __func__, start == nullptr ? "start" : "out_col");
        return TFGX_ERR_INVALID_ARG;
    }
    sample_from_kernel<<<grid_for(num_samples, kBlock), kBlock, 0, stream>>>(start, num_samples, uint64_t(num_nodes), adj_ptr,
                                                                             adj_col, seed, slot_base, max_attempts, out_col,
                                                                             n_failed);
    TFGX_LAUNCH_CHECK("sample_from_kernel");
    return TFGX_OK;
}
