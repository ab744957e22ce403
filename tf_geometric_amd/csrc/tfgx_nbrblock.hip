// Minibatch neighbour sampling (include/tfgx_nbrblock.h): a row-list sampler and an order-stable relabel over a persistent
// table — every launch is sized by the batch (n_rows, E), never by the graph.
//
// Reference: tf_geometric/utils/graph_utils.py:630-772 (RandomNeighborSampler), demo/demo_graph_sage.py (a block per layer).
//
// The sampler is the ListedRows instance of tfgx_sample_rows.h's kernel pair (tfgx_sample_neighbors is another): the generator
// keyed by the GLOBAL node id rows[i], the output offset out_ptr[i] — same bits as the whole-graph sampler, row by row.
//
// The relabel is four launches over the E sampled ids with a kernel boundary between any two that hand data on (nothing is
// passed between workgroups inside a launch):
//   mark    : atomicMin(table[c], n_known + p).  A known id's entry is < n_known and stays; a new id ends with
//             n_known + (its first position) whatever order the atomics land in (min is commutative).
//   flag    : first[p] = (table[cols[p]] == n_known + p), then one exclusive scan first -> rank (hipcub).
//   emit    : out_vcol[p] = entry < n_known ? entry : n_known + rank[entry - n_known]; a first occurrence also appends its id
//             to node_list; the last position writes *n_new.  The table is only read.
//   settle  : a first occurrence replaces its table entry by the virtual id (plain store, one writer per entry).
#include "tfgx_common.h"
#include "tfgx_host.h"
#include "tfgx_sample_rows.h"
#include "../../include/tfgx_nbrblock.h"

namespace tfgx {
namespace {

constexpr int32_t kEmpty = TFGX_NBRBLOCK_EMPTY;

__global__ void stamp_kernel(int32_t* __restrict__ table, int32_t n_nodes, const int32_t* __restrict__ ids, int64_t n,
                             int32_t base, int32_t* __restrict__ flag)
{
    int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; j < n; j += stride) {
        const int32_t c = ids[j];
        if (c < 0 || c >= n_nodes) {
            atomicOr(flag, TFGX_NBRBLOCK_BAD_RANGE);
            continue;
        }
        // exactly one of several stamps of one id finds the entry empty; the others (and a stamp over an older entry) report
        if (atomicCAS(&table[c], kEmpty, base + int32_t(j)) != kEmpty) atomicOr(flag, TFGX_NBRBLOCK_BAD_REPEAT);
    }
}

__global__ void relabel_mark_kernel(int32_t* __restrict__ table, int32_t n_nodes, int32_t n_known,
                                    const int32_t* __restrict__ cols, int64_t E)
{
    int64_t p = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; p < E; p += stride) {
        const int32_t c = cols[p];
        if (c < 0 || c >= n_nodes) continue;
        atomicMin(&table[c], n_known + int32_t(p));
    }
}

__global__ void relabel_flag_kernel(const int32_t* __restrict__ table, int32_t n_nodes, int32_t n_known,
                                    const int32_t* __restrict__ cols, int64_t E, int32_t* __restrict__ first)
{
    int64_t p = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; p < E; p += stride) {
        const int32_t c = cols[p];
        first[p] = (c >= 0 && c < n_nodes && table[c] == n_known + int32_t(p)) ? 1 : 0;
    }
}

__global__ void relabel_emit_kernel(const int32_t* __restrict__ table, int32_t n_nodes, int32_t n_known,
                                    const int32_t* __restrict__ cols, int64_t E, const int32_t* __restrict__ first,
                                    const int32_t* __restrict__ rank, int32_t* __restrict__ out_vcol,
                                    int32_t* __restrict__ node_list, int32_t* __restrict__ n_new)
{
    int64_t p = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; p < E; p += stride) {
        const int32_t c = cols[p];
        if (p == E - 1) *n_new = rank[p] + first[p];
        if (c < 0 || c >= n_nodes) {
            out_vcol[p] = -1;
            continue;
        }
        const int32_t t = table[c];
        if (t < n_known) {
            out_vcol[p] = t;
            continue;
        }
        const int32_t v = n_known + rank[t - n_known];              // t - n_known: the id's first position, in [0, p]
        out_vcol[p] = v;
        if (first[p]) node_list[v] = c;
    }
}

// after emit: out_vcol of a first occurrence is the id's virtual id; its entry still holds n_known + position
__global__ void relabel_settle_kernel(int32_t* __restrict__ table, const int32_t* __restrict__ cols, int64_t E,
                                      const int32_t* __restrict__ first, const int32_t* __restrict__ out_vcol)
{
    int64_t p = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; p < E; p += stride)
        if (first[p]) table[cols[p]] = out_vcol[p];
}

__global__ void reset_kernel(int32_t* __restrict__ table, int32_t n_nodes, const int32_t* __restrict__ node_list, int64_t n)
{
    int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; j < n; j += stride) {
        const int32_t c = node_list[j];
        if (c >= 0 && c < n_nodes) table[c] = kEmpty;
    }
}

// the relabel's workspace: first [E], rank [E], the scan's scratch
Workspace<3> relabel_workspace(int64_t E)
{
    return {{sizeof(int32_t) * size_t(E), sizeof(int32_t) * size_t(E), scan_bytes(E)}};
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_nbrblock_version(void) { return TFGX_NBRBLOCK_ABI_VERSION; }

extern "C" int tfgx_nbrblock_sample_rows(const int32_t* row_ptr, const int32_t* col, const float* w, int64_t n_nodes,
                                         const int32_t* rows, int64_t n_rows, const int32_t* out_ptr,
                                         int32_t replace_when_short, uint64_t seed, int32_t* out_col, float* out_w,
                                         int32_t* bad_flag, tfgx_stream_t stream)
{
    TFGX_RANGE();
    if (int rc = check_size(__func__, "n_nodes", n_nodes)) return rc;
    if (int rc = check_size(__func__, "n_rows", n_rows)) return rc;
    if (n_rows == 0) return TFGX_OK;
    if (rows == nullptr) return null_arg(__func__, "rows");
    if (out_ptr == nullptr) return null_arg(__func__, "out_ptr");
    if (bad_flag == nullptr) return null_arg(__func__, "bad_flag");
    if (n_nodes > 0 && row_ptr == nullptr) return null_arg(__func__, "row_ptr");
    if (n_nodes > 0 && col == nullptr) return null_arg(__func__, "col");
    if (n_nodes > 0 && out_col == nullptr) return null_arg(__func__, "out_col");
    const ListedRows listed{rows, int32_t(n_nodes), bad_flag, TFGX_NBRBLOCK_BAD_RANGE, seed};
    return launch_sample_rows(row_ptr, col, w, listed, n_rows, out_ptr, replace_when_short, out_col, out_w, as_stream(stream));
}

extern "C" int tfgx_nbrblock_stamp(int32_t* table, int64_t n_nodes, const int32_t* ids, int64_t n, int64_t base, int32_t* flag,
                                   tfgx_stream_t stream)
{
    TFGX_RANGE();
    if (int rc = check_size(__func__, "n_nodes", n_nodes)) return rc;
    if (int rc = check_size(__func__, "n", n)) return rc;
    if (int rc = check_size(__func__, "base", base)) return rc;
    if (base + n >= kMaxSize) {
        set_error("%s: base + n = %lld does not fit int32", __func__, (long long)(base + n));
        return TFGX_ERR_INVALID_ARG;
    }
    if (n == 0) return TFGX_OK;
    if (table == nullptr) return null_arg(__func__, "table");
    if (ids == nullptr) return null_arg(__func__, "ids");
    if (flag == nullptr) return null_arg(__func__, "flag");
    stamp_kernel<<<grid_for(n, kBlock), kBlock, 0, as_stream(stream)>>>(table, int32_t(n_nodes), ids, n, int32_t(base), flag);
    TFGX_LAUNCH_CHECK("stamp_kernel");
    return TFGX_OK;
}

extern "C" size_t tfgx_nbrblock_relabel_workspace_bytes(int64_t E)
{
    if (E <= 0 || E >= kMaxSize) return 0;
    return relabel_workspace(E).bytes();
}

extern "C" int tfgx_nbrblock_relabel(int32_t* table, int64_t n_nodes, int64_t n_known, const int32_t* cols, int64_t E,
                                     int32_t* out_vcol, int32_t* node_list, int32_t* n_new, void* workspace,
                                     size_t workspace_bytes, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_size(__func__, "n_nodes", n_nodes)) return rc;
    if (int rc = check_size(__func__, "n_known", n_known)) return rc;
    if (int rc = check_size(__func__, "E", E)) return rc;
    if (n_known + E >= kMaxSize) {       // the table keeps n_known + position below TFGX_NBRBLOCK_EMPTY
        set_error("%s: n_known + E = %lld does not fit int32", __func__, (long long)(n_known + E));
        return TFGX_ERR_INVALID_ARG;
    }
    if (E == 0) return TFGX_OK;          // nothing is written, *n_new included
    if (table == nullptr) return null_arg(__func__, "table");
    if (cols == nullptr) return null_arg(__func__, "cols");
    if (out_vcol == nullptr) return null_arg(__func__, "out_vcol");
    if (node_list == nullptr) return null_arg(__func__, "node_list");
    if (n_new == nullptr) return null_arg(__func__, "n_new");
    if (workspace == nullptr) return null_arg(__func__, "workspace");
    if (workspace_bytes < tfgx_nbrblock_relabel_workspace_bytes(E)) {
        set_error("%s: workspace_bytes = %zu is smaller than tfgx_nbrblock_relabel_workspace_bytes(E) = %zu", __func__,
                  workspace_bytes, tfgx_nbrblock_relabel_workspace_bytes(E));
        return TFGX_ERR_WORKSPACE;
    }
    const Workspace<3> ws = relabel_workspace(E);
    int32_t* first = ws.at<int32_t>(workspace, 0);
    int32_t* rank = ws.at<int32_t>(workspace, 1);
    void* temp = ws.at(workspace, 2);
    size_t temp_bytes = ws.piece[2];

    const int grid = grid_for(E, kBlock);
    relabel_mark_kernel<<<grid, kBlock, 0, stream>>>(table, int32_t(n_nodes), int32_t(n_known), cols, E);
    TFGX_LAUNCH_CHECK("relabel_mark_kernel");
    relabel_flag_kernel<<<grid, kBlock, 0, stream>>>(table, int32_t(n_nodes), int32_t(n_known), cols, E, first);
    TFGX_LAUNCH_CHECK("relabel_flag_kernel");
    TFGX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, first, rank, static_cast<int>(E), stream));
    relabel_emit_kernel<<<grid, kBlock, 0, stream>>>(table, int32_t(n_nodes), int32_t(n_known), cols, E, first, rank, out_vcol,
                                                     node_list, n_new);
    TFGX_LAUNCH_CHECK("relabel_emit_kernel");
    relabel_settle_kernel<<<grid, kBlock, 0, stream>>>(table, cols, E, first, out_vcol);
    TFGX_LAUNCH_CHECK("relabel_settle_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_nbrblock_reset(int32_t* table, int64_t n_nodes, const int32_t* node_list, int64_t n, tfgx_stream_t stream)
{
    TFGX_RANGE();
    if (int rc = check_size(__func__, "n_nodes", n_nodes)) return rc;
    if (int rc = check_size(__func__, "n", n)) return rc;
    if (n == 0) return TFGX_OK;
    if (table == nullptr) return null_arg(__func__, "table");
    if (node_list == nullptr) return null_arg(__func__, "node_list");
    reset_kernel<<<grid_for(n, kBlock), kBlock, 0, as_stream(stream)>>>(table, int32_t(n_nodes), node_list, n);
    TFGX_LAUNCH_CHECK("reset_kernel");
    return TFGX_OK;
}
