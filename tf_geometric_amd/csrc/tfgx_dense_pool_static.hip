// The pooled batch of one fixed-shape DiffPool / MinCutPool level (include/tfgx_dense_pool_static.h, where the layout is written
// down): the diagonal blocks P of S^T A S in, a static batch out.  Every launch is sized by capacities the host knows; the live
// totals (m_live, e_live) are read from device memory by the kernels that need them, never by the host.
//
// Reference: tf_geometric/nn/pool/diff_pool.py:8-105, nn/pool/min_cut_pool.py:127-143, utils/graph_utils.py:272-284.
//
// K <= 64 = one wave: lane c2 of a wave holds column c2 of row c1 of a slot's block, so the non-zero mask of the row is ONE ballot.
// count : one workgroup per slot, wave w takes rows w, w + 4, ...; the popcounts of the ballots are the slot's edges.
// scan  : ONE workgroup of kScanBlock threads, thread t owns a contiguous run of slots (tfgx_compact.h's scan and runs): the
//         live slots before a slot give its first pooled row, the kept entries before it its first pooled edge.
// emit  : one workgroup per slot.  The ballots go to LDS as 64 row words; wave 0 transposes them into 64 column words and scans
//         the popcounts of both (shuffles).  Entry (c1, c2) then lands at
//             e0 + row_off[c1] + popcount(row_bits[c1] below c2)     in the list and in the plan by row,
//             e0 + col_off[c2] + popcount(col_bits[c2] below c1)     in the plan by column (a stable sort by column keeps the
//         row-major order inside a column: column-major).  1.5 KiB of LDS, every LDS read a broadcast or one word per lane.
//         Behind the slots two fill sections: the dead and sink rows (with their row_ptr in closed form), the padded tail.
// No global atomics, no float atomics: every output is a pure function of the inputs.
#include "tfgx_common.h"
#include "tfgx_host.h"
#include "tfgx_compact.h"
#include "../../include/tfgx_dense_pool_static.h"

namespace tfgx {
namespace {

using namespace compact;

constexpr int kMaxK = TFGX_DENSE_POOL_STATIC_MAX_K;
constexpr int kFillTile = kBlock * 4;                  // rows / edges per workgroup of the fill sections
static_assert(kMaxK == kWave, "a row of a block is one wave ballot");

struct PlanOut {
    int32_t* row_ptr;
    int32_t* col;
    int32_t* perm;
};

struct Params {
    const float* P;
    int64_t ldp;
    const uint8_t* mask;
    const int32_t* parent_counts;
    int32_t B, K, drop_diagonal;
    int32_t n_cap_out, e_cap, sinks, sink_degree;
    int32_t m_rows;                    // n_cap_out - sinks: the rows that can be live
    int32_t row_tiles;                 // workgroups of the row fill section
    int32_t* prp;
    int32_t* node_index;
    int32_t* ngi;
    int32_t* node_map;
    int32_t* out_row;
    int32_t* out_col;
    int32_t* out_src;
    int32_t* out_egi;
    PlanOut plan[2];                   // by row, by column
    int32_t* counts;
    int32_t* slot_cnt;                 // [B]
    int32_t* slot_off;                 // [B + 1]
};

__device__ __forceinline__ uint64_t below(int lane) { return (uint64_t(1) << lane) - 1; }

// The non-zero mask of row c1 of slot g's block: bit c2 = "entry (c1, c2) is a pooled edge".  Lanes at and beyond K load the
// row's last column (a clamped load, not a predicated one) and drop out of the ballot.
__device__ __forceinline__ uint64_t row_mask(const Params& p, int32_t g, int32_t c1, int lane)
{
    const int32_t c2 = min(lane, p.K - 1);
    const float v = p.P[(int64_t(g) * p.K + c1) * p.ldp + c2];
    const bool keep = lane < p.K && v != 0.0f && !(p.drop_diagonal != 0 && c1 == c2);
    return __ballot(keep);
}

__global__ void __launch_bounds__(kBlock) dense_count_kernel(const Params p)
{
    __shared__ int32_t wave_cnt[kWavesPerBlock];
    const int32_t g = int32_t(blockIdx.x);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int32_t cnt = 0;
    if (p.mask[g] != 0)                                 // workgroup-uniform
        for (int32_t c1 = wave; c1 < p.K; c1 += kWavesPerBlock) cnt += __popcll(row_mask(p, g, c1, lane));
    if (lane == 0) wave_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t t = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) t += wave_cnt[w];
        p.slot_cnt[g] = t;
    }
}

__global__ void __launch_bounds__(kScanBlock) dense_scan_kernel(const Params p)
{
    const auto [begin, end] = thread_run(p.B);
    const int32_t kk = p.K * p.K;
    int64_t live = 0, edges = 0;
    for (int32_t j = begin; j < end; ++j) {
        live += p.mask[j] != 0 ? 1 : 0;
        edges += clampi(p.slot_cnt[j], 0, kk);
    }
    int64_t live_total, edge_total;
    int64_t live_run = block_exclusive_scan(live, live_total);
    int64_t edge_run = block_exclusive_scan(edges, edge_total);
    for (int32_t j = begin; j < end; ++j) {
        p.prp[j] = int32_t(min(live_run * p.K, int64_t(p.m_rows)));
        p.slot_off[j] = int32_t(min(edge_run, int64_t(p.e_cap)));
        live_run += p.mask[j] != 0 ? 1 : 0;
        edge_run += clampi(p.slot_cnt[j], 0, kk);
    }
    if (threadIdx.x == 0) {
        const int32_t m_live = int32_t(min(live_total * p.K, int64_t(p.m_rows)));
        const int32_t e_live = int32_t(min(edge_total, int64_t(p.e_cap)));
        p.prp[p.B] = m_live;
        p.prp[p.B + 1] = p.n_cap_out;
        p.slot_off[p.B] = e_live;
        p.counts[0] = p.parent_counts[0];
        p.counts[1] = m_live;
        p.counts[2] = e_live;
        p.counts[3] = p.parent_counts[3];
    }
}

// sections: [0, B) the slots; [B, B + row_tiles) the dead and sink rows; behind them the padded tail
__global__ void __launch_bounds__(kBlock) dense_emit_kernel(const Params p)
{
    __shared__ uint64_t row_bits[kMaxK], col_bits[kMaxK];
    __shared__ int32_t row_off[kMaxK], col_off[kMaxK];
    const int32_t b = int32_t(blockIdx.x);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int32_t K = p.K;
    // the live totals, held to the capacities whatever the tables say: no store leaves the outputs
    const int32_t m_live = clampi(p.prp[p.B], 0, p.m_rows);
    const int32_t e_live = clampi(p.slot_off[p.B], 0, p.e_cap);
    if (b < p.B) {
        const int32_t p0 = clampi(p.prp[b], 0, m_live);
        const bool live = p.mask[b] != 0 && p0 <= m_live - K;       // workgroup-uniform; rows [p0, p0 + K) are inside [0, m_live)
        if (!live) {
            if (int32_t(threadIdx.x) < K) p.node_map[int64_t(b) * K + threadIdx.x] = -1;
            return;
        }
        const int32_t e0 = clampi(p.slot_off[b], 0, e_live), e1 = clampi(p.slot_off[b + 1], e0, e_live);
        for (int32_t c1 = wave; c1 < K; c1 += kWavesPerBlock) {
            const uint64_t bits = row_mask(p, b, c1, lane);
            if (lane == 0) row_bits[c1] = bits;
        }
        __syncthreads();
        if (wave == 0) {
            // column `lane` of the bit matrix; the popcounts of row `lane` and column `lane`, scanned over the lanes
            uint64_t cb = 0;
            for (int32_t c1 = 0; c1 < K; ++c1) cb |= ((row_bits[c1] >> lane) & 1) << c1;      // a broadcast read
            const int32_t rc = lane < K ? __popcll(row_bits[min(lane, K - 1)]) : 0, cc = __popcll(cb);
            int32_t ri = rc, ci = cc;
#pragma unroll
            for (int off = 1; off < kWave; off <<= 1) {
                const int32_t ru = __shfl_up(ri, off, kWave), cu = __shfl_up(ci, off, kWave);
                if (lane >= off) ri += ru, ci += cu;
            }
            col_bits[lane] = cb;
            row_off[lane] = ri - rc;
            col_off[lane] = ci - cc;
        }
        __syncthreads();
        if (int32_t(threadIdx.x) < K) {
            const int32_t c = threadIdx.x, r = p0 + c;
            p.node_index[r] = b * K + c;
            p.ngi[r] = b;
            p.node_map[int64_t(b) * K + c] = r;
            p.plan[0].row_ptr[r] = min(e0 + row_off[c], e1);
            p.plan[1].row_ptr[r] = min(e0 + col_off[c], e1);
        }
        for (int32_t c1 = wave; c1 < K; c1 += kWavesPerBlock) {
            const uint64_t rb = row_bits[c1];
            if (((rb >> lane) & 1) == 0) continue;
            const int32_t c2 = lane;
            const int32_t q = e0 + row_off[c1] + __popcll(rb & below(c2));
            const int32_t qt = e0 + col_off[c2] + __popcll(col_bits[c2] & below(c1));
            if (q >= e1 || qt >= e1) continue;          // cannot happen while count and emit see the same P: held anyway
            p.out_row[q] = p0 + c1;
            p.out_col[q] = p0 + c2;
            p.out_src[q] = (b * K + c1) * K + c2;
            p.out_egi[q] = b;
            p.plan[0].col[q] = p0 + c2;
            p.plan[0].perm[q] = q;
            p.plan[1].col[qt] = p0 + c1;
            p.plan[1].perm[qt] = q;
        }
    } else if (b < p.B + p.row_tiles) {
        // rows [m_live, n_cap_out) are dead; row_ptr of rows [m_live, m_rows] is e_live, of row m_rows + t (t in [0, sinks]) the
        // start of sink t: it holds the padded edges [t, t + 1) * sink_degree of the tail
#pragma unroll
        for (int it = 0; it < kFillTile / kBlock; ++it) {
            const int64_t j = int64_t(b - p.B) * kFillTile + it * kBlock + threadIdx.x;
            if (j < m_live || j > p.n_cap_out) continue;
            if (j < p.n_cap_out) {
                p.node_index[j] = -1;
                p.ngi[j] = p.B;
            }
            const int64_t t = max(j - int64_t(p.m_rows), int64_t(0));
            const int32_t at = e_live + int32_t(min(int64_t(p.e_cap - e_live), t * p.sink_degree));
            p.plan[0].row_ptr[j] = at;
            p.plan[1].row_ptr[j] = at;
        }
    } else {
#pragma unroll
        for (int it = 0; it < kFillTile / kBlock; ++it) {
            const int64_t q64 = int64_t(b - p.B - p.row_tiles) * kFillTile + it * kBlock + threadIdx.x;
            if (q64 < e_live || q64 >= p.e_cap) continue;
            const int32_t q = int32_t(q64);
            const int32_t v = p.m_rows + (q - e_live) / p.sink_degree;      // < n_cap_out: sinks * sink_degree >= e_cap
            p.out_row[q] = v;
            p.out_col[q] = v;
            p.out_src[q] = -1;
            p.out_egi[q] = p.B;
            for (int k = 0; k < 2; ++k) {                                   // its own CSR position in both plans
                p.plan[k].col[q] = v;
                p.plan[k].perm[q] = q;
            }
        }
    }
}

Workspace<2> dense_workspace(int64_t B) { return Workspace<2>{{4 * size_t(B > 0 ? B : 1), 4 * size_t(B + 1)}}; }

int check_plan_out(const char* fn, const char* which, const tfgx_collate_plan* pl, int64_t e_cap)
{
    if (pl == nullptr) return null_arg(fn, which);
    const char* bad = nullptr;
    if (pl->out_row_ptr == nullptr) bad = "out_row_ptr";
    else if (e_cap > 0 && pl->out_col == nullptr) bad = "out_col";
    else if (e_cap > 0 && pl->out_perm == nullptr) bad = "out_perm";
    if (bad == nullptr) return TFGX_OK;
    set_error("%s: %s->%s is null", fn, which, bad);
    return TFGX_ERR_INVALID_ARG;
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_dense_pool_static_version(void) { return TFGX_DENSE_POOL_STATIC_ABI_VERSION; }

extern "C" size_t tfgx_dense_pool_static_workspace_bytes(int64_t B)
{
    if (B < 0 || B > TFGX_DENSE_POOL_STATIC_MAX_SLOTS) return 0;
    return dense_workspace(B).bytes();
}

extern "C" int tfgx_dense_pool_static(const tfgx_dense_pool_static_args* a, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    const char* fn = "tfgx_dense_pool_static";
    if (a == nullptr) return null_arg(fn, "args");
    const NamedSize sizes[] = {{"B", a->B}, {"K", a->K}, {"ldp", a->ldp}, {"n_cap_out", a->n_cap_out}, {"e_cap", a->e_cap},
                               {"sinks", a->sinks}, {"sink_degree", a->sink_degree}};
    if (int rc = check_sizes(fn, sizes)) return rc;
    if (a->B > TFGX_DENSE_POOL_STATIC_MAX_SLOTS) {
        set_error("%s: B = %lld is more than the %d slots one workgroup scans", fn, (long long)a->B, TFGX_DENSE_POOL_STATIC_MAX_SLOTS);
        return TFGX_ERR_INVALID_ARG;
    }
    if (a->K < 1 || a->K > kMaxK) {
        set_error("%s: K = %lld is outside [1, %d] (TFGX_DENSE_POOL_STATIC_MAX_K)", fn, (long long)a->K, kMaxK);
        return TFGX_ERR_INVALID_ARG;
    }
    if (a->ldp < a->K) return bad_arg(fn, "ldp is smaller than K", a->ldp);
    if (int rc = check_sink_degree(fn, a->sink_degree)) return rc;
    if (int rc = check_sink_tail(fn, a->sinks, a->sink_degree, a->e_cap)) return rc;
    const int64_t bk = a->B * a->K;                       // below 2^26
    if (int rc = check_size(fn, "B * K * K", bk * a->K)) return rc;
    if (a->n_cap_out < bk + a->sinks) {
        set_error("%s: n_cap_out = %lld is smaller than B * K + sinks = %lld", fn, (long long)a->n_cap_out, (long long)(bk + a->sinks));
        return TFGX_ERR_INVALID_ARG;
    }
    // no slots, no rows and no edges, and nowhere to put the offsets of an empty batch: nothing exists to be written
    if (a->B == 0 && a->n_cap_out == 0 && a->e_cap == 0 && a->plan == nullptr && a->plan_t == nullptr && a->counts == nullptr &&
        a->pooled_row_ptr == nullptr)
        return TFGX_OK;
    if (int rc = check_plan_out(fn, "plan", a->plan, a->e_cap)) return rc;
    if (int rc = check_plan_out(fn, "plan_t", a->plan_t, a->e_cap)) return rc;
    const char* bad = nullptr;
    if (a->counts == nullptr) bad = "counts";
    else if (a->parent_counts == nullptr) bad = "parent_counts";
    else if (a->pooled_row_ptr == nullptr) bad = "pooled_row_ptr";
    else if (a->workspace == nullptr) bad = "workspace";
    else if (a->B > 0 && a->P == nullptr) bad = "P";
    else if (a->B > 0 && a->graph_mask == nullptr) bad = "graph_mask";
    else if (a->B > 0 && a->node_map == nullptr) bad = "node_map";
    else if (a->n_cap_out > 0 && a->node_index == nullptr) bad = "node_index";
    else if (a->n_cap_out > 0 && a->node_graph_index == nullptr) bad = "node_graph_index";
    else if (a->e_cap > 0 && a->out_row == nullptr) bad = "out_row";
    else if (a->e_cap > 0 && a->out_col == nullptr) bad = "out_col";
    else if (a->e_cap > 0 && a->out_edge_src == nullptr) bad = "out_edge_src";
    else if (a->e_cap > 0 && a->out_edge_graph_index == nullptr) bad = "out_edge_graph_index";
    if (bad != nullptr) return null_arg(fn, bad);
    const Workspace<2> ws = dense_workspace(a->B);
    if (a->workspace_bytes < ws.bytes()) {
        set_error("%s: workspace_bytes = %zu is smaller than the %zu bytes tfgx_dense_pool_static_workspace_bytes asks for", fn,
                  a->workspace_bytes, ws.bytes());
        return TFGX_ERR_WORKSPACE;
    }

    Params p = {};
    p.P = a->P, p.ldp = a->ldp, p.mask = a->graph_mask, p.parent_counts = a->parent_counts;
    p.B = int32_t(a->B), p.K = int32_t(a->K), p.drop_diagonal = a->drop_diagonal;
    p.n_cap_out = int32_t(a->n_cap_out), p.e_cap = int32_t(a->e_cap), p.sinks = int32_t(a->sinks);
    p.sink_degree = int32_t(a->sink_degree);
    p.m_rows = int32_t(a->n_cap_out - a->sinks);
    p.row_tiles = int32_t((a->n_cap_out + 1 + kFillTile - 1) / kFillTile);
    p.prp = a->pooled_row_ptr, p.node_index = a->node_index, p.ngi = a->node_graph_index, p.node_map = a->node_map;
    p.out_row = a->out_row, p.out_col = a->out_col, p.out_src = a->out_edge_src, p.out_egi = a->out_edge_graph_index;
    p.plan[0] = PlanOut{a->plan->out_row_ptr, a->plan->out_col, a->plan->out_perm};
    p.plan[1] = PlanOut{a->plan_t->out_row_ptr, a->plan_t->out_col, a->plan_t->out_perm};
    p.counts = a->counts;
    p.slot_cnt = ws.at<int32_t>(a->workspace, 0);
    p.slot_off = ws.at<int32_t>(a->workspace, 1);

    if (p.B > 0) {
        dense_count_kernel<<<static_cast<unsigned>(p.B), kBlock, 0, stream>>>(p);
        TFGX_LAUNCH_CHECK("dense_count_kernel");
    }
    dense_scan_kernel<<<1, kScanBlock, 0, stream>>>(p);
    TFGX_LAUNCH_CHECK("dense_scan_kernel");
    const int64_t edge_tiles = (a->e_cap + kFillTile - 1) / kFillTile;
    const int64_t grid = int64_t(p.B) + p.row_tiles + edge_tiles;      // each term is below 2^31 / 1024 or 2^20
    dense_emit_kernel<<<static_cast<unsigned>(grid), kBlock, 0, stream>>>(p);
    TFGX_LAUNCH_CHECK("dense_emit_kernel");
    return TFGX_OK;
}
