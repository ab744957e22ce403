// Fixed-shape minibatch sampling (include/tfgx_nbrstatic.h): the seeds, one hop per call, the by-source plan of a block and
// the gather with dead rows — every size a launch needs is a capacity the host knows, every run-time size is read from device
// memory, nothing is read back.
//
// Reference: tf_geometric/utils/graph_utils.py:630-772 (RandomNeighborSampler), demo/demo_graph_sage.py (a block per layer).
//
// A hop is a fixed sequence on the one given stream, with a kernel boundary between any two launches that hand data on:
//   count   : cnt[i] = draws of row i from row_ptr[node[i]], 0 for a dead row (and for the extra entry R); the candidate id
//             list is filled with -1 (what the relabel skips).
//   scan    : ONE exclusive sum cnt -> block_row_ptr[0 .. R]; block_row_ptr[R] is the hop's edge total.
//   sample  : the kernel pair of tfgx_sample_rows.h (the one tfgx_nbrblock_sample_rows launches: a lane per short row, a wave
//             per long one), its ListedRowsDeviceSeed instance: keyed by the global id, the seed mixed from the device word.
//   relabel : tfgx_nbrblock_relabel over the E candidate slots with n_known = R: new ids take R, R + 1, ... in first-occurrence
//             order (integer atomicMin, flags, a scan), their global ids land in node[R ...], counts[1] = how many.
//   finish  : row positions of the sampled edges (a binary search in block_row_ptr), the tail self-loops on the sinks with unit
//             weights, block_row_ptr past R in closed form, -1 for the unused slots and the sinks of `node`, counts[0].
// The other entry of the header, tfgx_nbrstatic_input_hop_f32, is the seed-pointer form of samplereduce_kernel and lives in
// tfgx_samplereduce.hip.  The gather out of a 16-bit table (include/tfgx_minibatch_h16.h) sits next to the float32 one.
#include "tfgx_common.h"
#include "tfgx_host.h"
#include "tfgx_gather.h"
#include "tfgx_sample_rows.h"
#include "tfgx_widen_h16.h"
#include "../../include/tfgx_nbrblock.h"
#include "../../include/tfgx_nbrstatic.h"
#include "../../include/tfgx_minibatch_h16.h"

namespace tfgx {
namespace {

__global__ void seeds_mark_kernel(int32_t* __restrict__ table, int32_t n_nodes, const int32_t* __restrict__ seeds, int64_t B,
                                  int32_t* __restrict__ flag)
{
    int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; j < B; j += stride) {
        const int32_t s = seeds[j];
        if (s == TFGX_NBRSTATIC_DEAD) continue;
        if (s < 0 || s >= n_nodes) {
            atomicOr(flag, TFGX_NBRSTATIC_BAD_RANGE);
            continue;
        }
        atomicMin(&table[s], int32_t(j));          // the first occurrence wins whatever order the lanes arrive in
    }
}

__global__ void seeds_settle_kernel(const int32_t* __restrict__ table, int32_t n_nodes, const int32_t* __restrict__ seeds,
                                    int64_t B, int32_t* __restrict__ node, int32_t* __restrict__ flag)
{
    int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; j < B; j += stride) {
        const int32_t s = seeds[j];
        int32_t v = TFGX_NBRSTATIC_DEAD;
        if (s >= 0 && s < n_nodes) {
            if (table[s] == int32_t(j)) v = s;
            else atomicOr(flag, TFGX_NBRSTATIC_BAD_REPEAT);
        }
        node[j] = v;
    }
}

// cnt [R + 1] (the last entry 0: the scan's total lands in block_row_ptr[R]) and the candidate list emptied
__global__ void hop_count_kernel(const int32_t* __restrict__ row_ptr, int32_t n_nodes, const int32_t* __restrict__ node,
                                 int64_t R, int k, int replace_when_short, int64_t E, int32_t* __restrict__ cnt,
                                 int32_t* __restrict__ gcol)
{
    const int64_t t0 = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = t0; i <= R; i += stride) {
        int m = 0;
        if (i < R) {
            const int32_t r = node[i];
            if (r >= 0 && r < n_nodes) m = sample_row_draws(row_ptr[r + 1] - row_ptr[r], k, replace_when_short);
        }
        cnt[i] = m;
    }
    for (int64_t p = t0; p < E; p += stride) gcol[p] = -1;
}

// after the relabel: block_col[0 .. total) and node[R .. R + n_new) are written, counts[1] = n_new
__global__ void hop_finish_kernel(int64_t R, int k, int64_t E, int64_t S, int32_t* __restrict__ block_row_ptr,
                                  int32_t* __restrict__ block_row, int32_t* __restrict__ block_col,
                                  float* __restrict__ block_w, int32_t* __restrict__ node, int32_t* __restrict__ counts)
{
    const int64_t t0 = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int32_t total = block_row_ptr[R];             // entries [0, R] are only read here
    const int32_t n_new = counts[1];
    const int64_t tail = E - total;
    for (int64_t p = t0; p < E; p += stride) {
        if (p < total) {
            int64_t lo = 0, hi = R;                       // the row i with block_row_ptr[i] <= p < block_row_ptr[i + 1]
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) / 2;
                if (block_row_ptr[mid] <= p) lo = mid;
                else hi = mid;
            }
            block_row[p] = int32_t(lo);
        } else {
            const int32_t v = int32_t(R + E + (p - total) / k);      // (p - total) / k < S: tail <= E = R * k
            block_row[p] = v;
            block_col[p] = v;
            block_w[p] = 1.0f;
        }
    }
    for (int64_t q = R + 1 + t0; q <= R + E + S; q += stride) {
        int64_t v = total;
        if (q > R + E) v += min(tail, (q - (R + E)) * int64_t(k));
        block_row_ptr[q] = int32_t(v);
    }
    for (int64_t v = R + n_new + t0; v < R + E + S; v += stride) node[v] = TFGX_NBRSTATIC_DEAD;
    if (t0 == 0) counts[0] = total;
}

__global__ void iota_kernel(int64_t n, int32_t* __restrict__ out)
{
    int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; i < n; i += stride) out[i] = int32_t(i);
}

// keys sorted ascending, every key in [0, n): row_ptr[v] = the first position whose key is >= v (tfgx_plan.hip's rule)
__global__ void row_ptr_of_sorted_kernel(const int32_t* __restrict__ keys, int64_t E, int32_t n, int32_t* __restrict__ row_ptr)
{
    int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; i <= E; i += stride) {
        const int32_t lo = (i == 0) ? 0 : keys[i - 1] + 1;
        const int32_t hi = (i == E) ? n : min(keys[i], n);
        for (int32_t v = max(lo, 0); v <= hi; ++v) row_ptr[v] = int32_t(i);
    }
}

// columns [col0, col0 + ncols * VEC) of every row: a lane per (row, chunk).  A dead row loads row 0 — a clamped address — and
// drops the value with a select once the load is issued: no load is predicated.
template <int VEC>
__global__ void gather_rows_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ idx, int64_t M,
                                   int col0, int ncols, float* __restrict__ out, int64_t ldo)
{
    int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t total = M * ncols;
    for (; t < total; t += stride) {
        const int64_t i = t / ncols;
        const int c = int(t - i * ncols);
        const int32_t id = idx[i];
        const int64_t row = id < 0 ? 0 : id;
        float v[VEC];
        load_vec<VEC>(x + row * ldx + col0 + int64_t(c) * VEC, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) asm volatile("" : "+v"(v[e]));
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = id < 0 ? 0.0f : v[e];
        store_vec<VEC>(out + i * ldo + col0 + int64_t(c) * VEC, v);
    }
}

// the same gather out of a 16-bit table (include/tfgx_minibatch_h16.h): a lane per (row, 16-byte chunk of 8 elements), widened in
// registers and stored as float32; the last chunk reads the row's pad columns and stores only the columns below F
template <int DT>
__global__ void gather_rows_h16_kernel(const uint16_t* __restrict__ x, int64_t ldx, const int32_t* __restrict__ idx, int64_t M,
                                       int F, int nchunks, float* __restrict__ out, int64_t ldo, int out_vec)
{
    int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t total = M * nchunks;
    for (; t < total; t += stride) {
        const int64_t i = t / nchunks;
        const int c = int(t - i * nchunks);
        const int32_t id = idx[i];
        const int64_t row = id < 0 ? 0 : id;
        uint4 raw = *reinterpret_cast<const uint4*>(x + row * ldx + int64_t(c) * kVec);
        asm volatile("" : "+v"(raw.x), "+v"(raw.y), "+v"(raw.z), "+v"(raw.w));
        float v[kVec];
        widen8<DT>(raw, v);
#pragma unroll
        for (int e = 0; e < kVec; ++e) v[e] = id < 0 ? 0.0f : v[e];
        store8_f32(out + i * ldo + int64_t(c) * kVec, out_vec != 0, min(kVec, F - c * kVec), v);
    }
}

size_t sort_bytes(int64_t E, int64_t n)
{
    size_t temp = 0;
    const int32_t* kin = nullptr;
    int32_t* kout = nullptr;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, temp, kin, kout, kin, kout, static_cast<int>(E > 0 ? E : 1), 0, key_bits(n));
    return temp;
}

// R' = R + R * k + (k > 0 ? R : 0), or -1 when it does not fit int32
int64_t hop_nodes(int64_t R, int32_t k)
{
    if (R < 0 || k < 0 || R >= kMaxSize) return -1;
    const int64_t total = R + R * int64_t(k) + (k > 0 ? R : 0);       // R < 2^31, k < 2^31: no int64 overflow
    return total >= kMaxSize ? -1 : total;
}

// a hop's workspace: cnt [R + 1], the candidate ids [E], the scan's scratch, the relabel's
Workspace<4> hop_workspace(int64_t R, int64_t E)
{
    return {{sizeof(int32_t) * size_t(R + 1), sizeof(int32_t) * size_t(E), scan_bytes(R + 1),
             tfgx_nbrblock_relabel_workspace_bytes(E)}};
}

// the transpose's workspace: the sorted keys [E], the positions [E], hipcub's own
Workspace<3> transpose_workspace(int64_t E, int64_t n)
{
    return {{sizeof(int32_t) * size_t(E), sizeof(int32_t) * size_t(E), sort_bytes(E, n)}};
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_nbrstatic_version(void) { return TFGX_NBRSTATIC_ABI_VERSION; }

extern "C" int tfgx_nbrstatic_seeds(int32_t* table, int64_t n_nodes, const int32_t* seeds, int64_t B, int32_t* node,
                                    int32_t* flag, tfgx_stream_t stream)
{
    TFGX_RANGE();
    if (int rc = check_size(__func__, "n_nodes", n_nodes)) return rc;
    if (int rc = check_size(__func__, "B", B)) return rc;
    if (B == 0) return TFGX_OK;
    if (seeds == nullptr) return null_arg(__func__, "seeds");
    if (node == nullptr) return null_arg(__func__, "node");
    if (flag == nullptr) return null_arg(__func__, "flag");
    if (n_nodes > 0 && table == nullptr) return null_arg(__func__, "table");
    const int grid = grid_for(B, kBlock);
    seeds_mark_kernel<<<grid, kBlock, 0, as_stream(stream)>>>(table, int32_t(n_nodes), seeds, B, flag);
    TFGX_LAUNCH_CHECK("seeds_mark_kernel");
    seeds_settle_kernel<<<grid, kBlock, 0, as_stream(stream)>>>(table, int32_t(n_nodes), seeds, B, node, flag);
    TFGX_LAUNCH_CHECK("seeds_settle_kernel");
    return TFGX_OK;
}

extern "C" size_t tfgx_nbrstatic_hop_workspace_bytes(int64_t R, int32_t k)
{
    if (R <= 0 || k <= 0 || hop_nodes(R, k) < 0) return 0;
    return hop_workspace(R, R * int64_t(k)).bytes();
}

extern "C" int tfgx_nbrstatic_hop(const int32_t* row_ptr, const int32_t* col, const float* w, int64_t n_nodes, int32_t* table,
                                  int32_t* node, int64_t R, int32_t k, int32_t replace_when_short, const uint64_t* seed,
                                  int32_t hop, int32_t* block_row_ptr, int32_t* block_row, int32_t* block_col, float* block_w,
                                  int32_t* counts, void* workspace, size_t workspace_bytes, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_size(__func__, "n_nodes", n_nodes)) return rc;
    if (int rc = check_size(__func__, "R", R)) return rc;
    if (k < 0) return bad_arg(__func__, "k must not be negative", k);
    if (hop < 0) return bad_arg(__func__, "hop must not be negative", hop);
    if (hop_nodes(R, k) < 0) {
        set_error("%s: R + R * k + sinks = %lld nodes do not fit int32", __func__,
                  (long long)(R + R * int64_t(k) + (k > 0 ? R : 0)));
        return TFGX_ERR_INVALID_ARG;
    }
    if (R == 0) return TFGX_OK;
    if (block_row_ptr == nullptr) return null_arg(__func__, "block_row_ptr");
    if (counts == nullptr) return null_arg(__func__, "counts");
    const int64_t E = R * int64_t(k), S = k > 0 ? R : 0;
    if (E == 0) {                       // no fan-out: an empty block on the R rows
        TFGX_HIP_CHECK(hipMemsetAsync(block_row_ptr, 0, sizeof(int32_t) * size_t(R + 1), stream));
        TFGX_HIP_CHECK(hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), stream));
        return TFGX_OK;
    }
    if (node == nullptr) return null_arg(__func__, "node");
    if (seed == nullptr) return null_arg(__func__, "seed");
    if (block_row == nullptr) return null_arg(__func__, "block_row");
    if (block_col == nullptr) return null_arg(__func__, "block_col");
    if (block_w == nullptr) return null_arg(__func__, "block_w");
    if (n_nodes > 0 && row_ptr == nullptr) return null_arg(__func__, "row_ptr");
    if (n_nodes > 0 && col == nullptr) return null_arg(__func__, "col");
    if (n_nodes > 0 && table == nullptr) return null_arg(__func__, "table");
    if (workspace == nullptr) return null_arg(__func__, "workspace");
    if (workspace_bytes < tfgx_nbrstatic_hop_workspace_bytes(R, k)) {
        set_error("%s: workspace_bytes = %zu is smaller than tfgx_nbrstatic_hop_workspace_bytes(R, k) = %zu", __func__,
                  workspace_bytes, tfgx_nbrstatic_hop_workspace_bytes(R, k));
        return TFGX_ERR_WORKSPACE;
    }
    const Workspace<4> ws = hop_workspace(R, E);
    int32_t* cnt = ws.at<int32_t>(workspace, 0);
    int32_t* gcol = ws.at<int32_t>(workspace, 1);
    void* scan_temp = ws.at(workspace, 2);
    size_t scan_temp_bytes = ws.piece[2];
    void* relabel_ws = ws.at(workspace, 3);
    const size_t relabel_bytes = ws.piece[3];

    hop_count_kernel<<<grid_for(E > R ? E : R + 1, kBlock), kBlock, 0, stream>>>(row_ptr, int32_t(n_nodes), node, R, k,
                                                                                 replace_when_short, E, cnt, gcol);
    TFGX_LAUNCH_CHECK("hop_count_kernel");
    TFGX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(scan_temp, scan_temp_bytes, cnt, block_row_ptr, static_cast<int>(R + 1),
                                                    stream));
    const ListedRowsDeviceSeed listed{node, int32_t(n_nodes), seed, hop};
    if (int rc = launch_sample_rows(row_ptr, col, w, listed, R, block_row_ptr, replace_when_short, gcol, block_w, stream)) return rc;
    // new ids are numbered R, R + 1, ... and appended to node[R ...]; the slots past the total hold -1 and are skipped
    if (int rc = tfgx_nbrblock_relabel(table, n_nodes, R, gcol, E, block_col, node, counts + 1, relabel_ws, relabel_bytes,
                                       stream_))
        return rc;
    hop_finish_kernel<<<grid_for(E + S + 1, kBlock), kBlock, 0, stream>>>(R, k, E, S, block_row_ptr, block_row, block_col,
                                                                          block_w, node, counts);
    TFGX_LAUNCH_CHECK("hop_finish_kernel");
    return TFGX_OK;
}

extern "C" size_t tfgx_nbrstatic_transpose_workspace_bytes(int64_t E, int64_t n)
{
    if (E <= 0 || n < 0 || E >= kMaxSize || n >= kMaxSize) return 0;
    return transpose_workspace(E, n).bytes();
}

extern "C" int tfgx_nbrstatic_transpose(const int32_t* block_row, const int32_t* block_col, int64_t E, int64_t n,
                                        int32_t* t_row_ptr, int32_t* t_col, int32_t* t_perm, void* workspace,
                                        size_t workspace_bytes, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_size(__func__, "E", E)) return rc;
    if (int rc = check_size(__func__, "n", n)) return rc;
    if (E == 0 && n == 0) return TFGX_OK;
    if (t_row_ptr == nullptr) return null_arg(__func__, "t_row_ptr");
    if (E == 0) {
        TFGX_HIP_CHECK(hipMemsetAsync(t_row_ptr, 0, sizeof(int32_t) * size_t(n + 1), stream));
        return TFGX_OK;
    }
    if (n == 0) return bad_arg(__func__, "edges over n = 0 nodes: E", (long long)E);
    if (block_row == nullptr) return null_arg(__func__, "block_row");
    if (block_col == nullptr) return null_arg(__func__, "block_col");
    if (t_col == nullptr) return null_arg(__func__, "t_col");
    if (t_perm == nullptr) return null_arg(__func__, "t_perm");
    if (workspace == nullptr) return null_arg(__func__, "workspace");
    if (workspace_bytes < tfgx_nbrstatic_transpose_workspace_bytes(E, n)) {
        set_error("%s: workspace_bytes = %zu is smaller than tfgx_nbrstatic_transpose_workspace_bytes(E, n) = %zu", __func__,
                  workspace_bytes, tfgx_nbrstatic_transpose_workspace_bytes(E, n));
        return TFGX_ERR_WORKSPACE;
    }
    const Workspace<3> ws = transpose_workspace(E, n);
    int32_t* keys_out = ws.at<int32_t>(workspace, 0);
    int32_t* iota = ws.at<int32_t>(workspace, 1);
    void* temp = ws.at(workspace, 2);
    size_t temp_bytes = ws.piece[2];

    const int grid = grid_for(E, kBlock);
    iota_kernel<<<grid, kBlock, 0, stream>>>(E, iota);
    TFGX_LAUNCH_CHECK("iota_kernel");
    // a stable LSD radix sort of (source, position): equal sources keep their block order
    TFGX_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, block_col, keys_out, iota, t_perm, static_cast<int>(E), 0,
                                                      key_bits(n), stream));
    gather_by_index<<<grid, kBlock, 0, stream>>>(block_row, t_perm, E, t_col);
    TFGX_LAUNCH_CHECK("gather_by_index");
    row_ptr_of_sorted_kernel<<<grid_for(E + 1, kBlock), kBlock, 0, stream>>>(keys_out, E, int32_t(n), t_row_ptr);
    TFGX_LAUNCH_CHECK("row_ptr_of_sorted_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_nbrstatic_gather_rows_f32(const float* x, int64_t ldx, const int32_t* idx, int64_t M, int64_t F, float* out,
                                              int64_t ldo, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_size(__func__, "M", M)) return rc;
    if (F < 1) return bad_arg(__func__, "F must be at least 1", (long long)F);
    if (int rc = check_size(__func__, "F", F)) return rc;
    if (ldx < F) return bad_arg(__func__, "ldx must be at least F", (long long)ldx);
    if (ldo < F) return bad_arg(__func__, "ldo must be at least F", (long long)ldo);
    if (M == 0) return TFGX_OK;
    if (x == nullptr) return null_arg(__func__, "x");
    if (idx == nullptr) return null_arg(__func__, "idx");
    if (out == nullptr) return null_arg(__func__, "out");
    const bool vec = F >= 4 && ldx % 4 == 0 && ldo % 4 == 0 && aligned_to(x, 16) && aligned_to(out, 16);
    if (vec) {
        const int nv = int(F / 4), tail = int(F - int64_t(nv) * 4);
        gather_rows_kernel<4><<<grid_for(M * nv, kBlock), kBlock, 0, stream>>>(x, ldx, idx, M, 0, nv, out, ldo);
        TFGX_LAUNCH_CHECK("gather_rows_kernel<4>");
        if (tail > 0) {
            gather_rows_kernel<1><<<grid_for(M * tail, kBlock), kBlock, 0, stream>>>(x, ldx, idx, M, nv * 4, tail, out, ldo);
            TFGX_LAUNCH_CHECK("gather_rows_kernel<1>");
        }
    } else {
        gather_rows_kernel<1><<<grid_for(M * F, kBlock), kBlock, 0, stream>>>(x, ldx, idx, M, 0, int(F), out, ldo);
        TFGX_LAUNCH_CHECK("gather_rows_kernel<1>");
    }
    return TFGX_OK;
}

// include/tfgx_minibatch_h16.h: the gather of both minibatch classes out of a 16-bit table (its other entries, the fused input
// hop over such a table, live in tfgx_samplereduce.hip)
extern "C" int tfgx_gather_rows_h16_f32(const void* x, int64_t ldx, int32_t x_dtype, const int32_t* idx, int64_t M, int64_t F,
                                        float* out, int64_t ldo, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (!is_h16(x_dtype)) return bad_arg(__func__, "x_dtype must be TFGX_DT_BF16 or TFGX_DT_F16", x_dtype);
    if (int rc = check_size(__func__, "M", M)) return rc;
    if (F < 1) return bad_arg(__func__, "F must be at least 1", (long long)F);
    if (int rc = check_size(__func__, "F", F)) return rc;
    if (ldx < F) return bad_arg(__func__, "ldx must be at least F", (long long)ldx);
    if (ldx % kVec != 0) return bad_arg(__func__, "ldx must be a multiple of 8: rows of a 16-bit table are 16-byte aligned", (long long)ldx);
    if (!aligned_to(x, 16)) return bad_arg(__func__, "x must be 16-byte aligned: its address modulo 16", (long long)(reinterpret_cast<uintptr_t>(x) % 16));
    if (ldo < F) return bad_arg(__func__, "ldo must be at least F", (long long)ldo);
    if (M == 0) return TFGX_OK;
    if (x == nullptr) return null_arg(__func__, "x");
    if (idx == nullptr) return null_arg(__func__, "idx");
    if (out == nullptr) return null_arg(__func__, "out");
    const int nchunks = int((F + kVec - 1) / kVec);
    const int out_vec = (ldo % 4 == 0 && aligned_to(out, 16)) ? 1 : 0;
    const uint16_t* xh = static_cast<const uint16_t*>(x);
    const int grid = grid_for(M * nchunks, kBlock);
    if (x_dtype == TFGX_DT_BF16) gather_rows_h16_kernel<TFGX_DT_BF16><<<grid, kBlock, 0, stream>>>(xh, ldx, idx, M, int(F), nchunks, out, ldo, out_vec);
    else gather_rows_h16_kernel<TFGX_DT_F16><<<grid, kBlock, 0, stream>>>(xh, ldx, idx, M, int(F), nchunks, out, ldo, out_vec);
    TFGX_LAUNCH_CHECK("gather_rows_h16_kernel");
    return TFGX_OK;
}
