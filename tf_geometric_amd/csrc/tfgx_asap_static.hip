// The three device pieces of one fixed-shape ASAP level (include/tfgx_asap_static.h, where the contracts are written down).
//
// Reference: tf_geometric/nn/pool/asap.py:67-85 (attention), :109-127 and nn/pool/cluster_pool.py:32-46 (assignment, S^T A S).
//
// attend : the kernel of tfgx_asap_attend.h with SKIP_LOOPS set by the flag; the seed may live in device memory.  Its backward
//          here is the centred form (above the kernel), which keeps the gradient of a row whose weights sum to 1.0f.
// assign : S is zeroed by a launch of its own; then a wave per pooled row r (centre i, column c of S).  The row of i is walked
//          64 edges at a time (chunk A: lane l owns edge a + l); for every chunk A the wave walks the WHOLE row again (chunk B) and broadcasts its edges one by one: a
//          lane adds the weights of the edges that share its column, in CSR order, and learns whether an earlier edge had that
//          column.  The lane of the first edge of a column stores the column's sum — once, no read-modify-write.  L * L / 64
//          steps for a row of L edges: rows of a static batch are short.
// edges  : K <= 64 = one wave: lane c2 of a wave holds column c2 of row c1 of a slot's block, so the mask of a row (its
//          off-diagonal non-zero entries below m_g, and its diagonal) is ONE ballot.
//          count : one workgroup per slot, wave w takes rows w, w + 4, ...; the popcounts are the slot's edges.
//          scan  : ONE workgroup of kScanBlock threads scans the B slots (tfgx_compact.h) and writes counts[2].
//          emit  : one workgroup per slot.  The ballots go to LDS as row words; wave 0 transposes them into column words and
//                  scans the popcounts of both.  Entry (c1, c2), c2 != c1, lands at
//                      e0 + row_off[c1] + popcount(row_bits[c1] without its diagonal, below c2)
//                  in the list and in the plan by row, the self-loop of row c1 behind the row's other entries, and either at
//                      e0 + col_off[c2] + popcount(col_bits[c2] below c1)
//                  in the plan by column (a stable sort by column keeps the list order inside a column, where the self-loop of
//                  c2 stands between the rows below and above c2).  Behind the slots two fill sections: the row_ptr of the dead
//                  and sink rows in closed form, the padded tail.
// No global atomics, no float atomics: every output is a pure function of the inputs.
#include "tfgx_common.h"
#include "tfgx_host.h"
#include "tfgx_compact.h"
#include "tfgx_asap_attend.h"
#include "../../include/tfgx_asap_static.h"

namespace tfgx {
namespace {

using namespace compact;

constexpr int kMaxK = TFGX_ASAPSTATIC_MAX_K;
constexpr int kFillTile = kBlock * 4;                  // rows / edges per workgroup of the fill sections
static_assert(kMaxK == kWave, "a row of a block is one wave ballot");

// ---- (b) the assignment -------------------------------------------------------------------------------------------------------
// S = 0 by a kernel of this file, so that a replayed hipGraph zeroes S again before every assignment.  lds == K (what
// nn.asap_static passes): one flat run, no division.
__global__ void __launch_bounds__(kBlock) asap_zero_kernel(float* __restrict__ S, int64_t total, int64_t K, int64_t lds)
{
    for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < total; j += int64_t(gridDim.x) * kBlock)
        S[lds == K ? j : (j / K) * lds + (j % K)] = 0.0f;
}

__global__ void __launch_bounds__(kBlock) asap_assign_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                             int32_t N, int32_t E, const float* __restrict__ p,
                                                             const float* __restrict__ p_self, int32_t skip,
                                                             const int32_t* __restrict__ node_index,
                                                             const int32_t* __restrict__ pooled_ngi,
                                                             const int32_t* __restrict__ prp, int32_t B, int32_t m_rows, int32_t K,
                                                             float* __restrict__ S, int64_t lds)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int32_t r = int32_t(blockIdx.x) * kWavesPerBlock + wave;      // wave-uniform
    if (r >= m_rows) return;
    const int32_t i = node_index[r], g = pooled_ngi[r];
    if (i < 0 || i >= N || g < 0 || g >= B) return;
    const int32_t c = r - prp[g];
    if (c < 0 || c >= K) return;
    int32_t beg = row_ptr[i], end = row_ptr[i + 1];
    if (!(beg >= 0 && end >= beg && end <= E)) beg = end = 0;
    const float ps = p_self[i];
    bool centre_seen = false;                              // wave-uniform: an edge that counts has the centre as its column
    for (int32_t a = beg; a < end; a += kWave) {
        const int32_t ea = a + lane;
        const bool act = ea < end;
        const int32_t ca = act ? col[ea] : -1;
        const bool mine = act && ca >= 0 && ca < N && !(skip != 0 && ca == i);
        bool first = mine;
        float sum = 0.0f;
        for (int32_t b = beg; b < end; b += kWave) {
            const int32_t eb = b + lane;
            const bool actb = eb < end;
            const int32_t cb = actb ? col[eb] : -1;
            const float pb = actb ? p[eb] : 0.0f;
            const int cnt = min(end - b, kWave);
            for (int k = 0; k < cnt; ++k) {
                const int32_t ck = __shfl(cb, k);
                const float pk = __shfl(pb, k);
                if (mine && ck == ca) {
                    sum += pk;                             // CSR order: b ascending, k ascending
                    if (b + k < ea) first = false;
                }
            }
        }
        if (mine && ca == i) sum += ps;                    // the centre's own weight comes last
        centre_seen = centre_seen || __any(mine && ca == i);
        if (mine && first) S[int64_t(ca) * lds + c] = sum;
    }
    if (!centre_seen && lane == 0) S[int64_t(i) * lds + c] = ps;
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- (a') the attention backward, centred ---------------------------------------------------------------------------------
// With u_e = k_e dp_e and r = u of the self edge, ds_e = p_e (u_e - sum_j p_j u_j) = p_e ((u_e - r) - sum_j p_j (u_j - r) + r eps / D):
// sum_j p_j = 1 - eps / D is never formed, so a row whose weights sum to 1.0f in float32 (one term: p_self = 1 / (1 + 1e-8))
// still gets the gradient the epsilon of the denominator leaves it.  m and D are recomputed from the scores (three walks).
__global__ void __launch_bounds__(kBlock) asap_attend_backward_centred_kernel(
    const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, int64_t N, int64_t E, const float* __restrict__ sq,
    const float* __restrict__ sh, const float* __restrict__ bias, const float* __restrict__ p, const float* __restrict__ p_self,
    const float* __restrict__ pd, const float* __restrict__ pd_self, const float* __restrict__ dp, const float* __restrict__ dp_self,
    int32_t dropped, int32_t skip, float* __restrict__ ds, float* __restrict__ ds_self, float* __restrict__ dsq)
{
    using asap_attend::kAlpha;
    using asap_attend::kEps;
    using asap_attend::leaky;
    using asap_attend::wave_max;
    using asap_attend::wave_sum;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const float b0 = *bias;
    // dropped == 0 (no dropout, pd / pd_self are p / p_self): k_e = 1, u_e = dp_e without a division
    for (int64_t row = int64_t(blockIdx.x) * kWavesPerBlock + wave; row < N; row += int64_t(gridDim.x) * kWavesPerBlock) {
        int64_t beg = row_ptr[row], end = row_ptr[row + 1];
        if (!(beg >= 0 && end >= beg && end <= E)) beg = end = 0;
        const float sqr = sq[row] + b0;
        const float z_self = sqr + sh[row], s_self = leaky(z_self);
        const double ps = p_self[row];
        const double r = !dropped ? double(dp_self[row]) : (ps > 0.0 ? (double(pd_self[row]) / ps) * double(dp_self[row]) : 0.0);
        float m = s_self;
        for (int64_t i = beg + lane; i < end; i += kWave) {
            const int32_t cj = col[i];
            const bool ok = cj >= 0 && int64_t(cj) < N && !(skip != 0 && int64_t(cj) == row);
            if (ok) m = fmaxf(m, leaky(sqr + sh[cj]));
        }
        m = wave_max(m);
        // the row sums are carried in double: dsq is a sum of ds over the row that cancels but for the slopes of leaky_relu
        double sum = 0.0, tdel = 0.0;
        for (int64_t i = beg + lane; i < end; i += kWave) {
            const int32_t cj = col[i];
            const bool ok = cj >= 0 && int64_t(cj) < N && !(skip != 0 && int64_t(cj) == row);
            if (!ok) continue;
            sum += double(expf(leaky(sqr + sh[cj]) - m));
            const double pe = p[i];
            if (pe > 0.0) tdel += pe * ((dropped ? (double(pd[i]) / pe) * double(dp[i]) : double(dp[i])) - r);
        }
        const double D = (wave_sum_f64(sum) + double(expf(s_self - m))) + double(kEps);
        const double base = r * (double(kEps) / D) - wave_sum_f64(tdel);
        double acc = 0.0;
        for (int64_t i = beg + lane; i < end; i += kWave) {
            const int32_t cj = col[i];
            const bool ok = cj >= 0 && int64_t(cj) < N && !(skip != 0 && int64_t(cj) == row);
            double v = 0.0;
            const double pe = p[i];
            if (ok && pe > 0.0) {
                const float z = sqr + sh[cj];
                v = pe * (((dropped ? (double(pd[i]) / pe) * double(dp[i]) : double(dp[i])) - r) + base) * (z > 0.0f ? 1.0 : double(kAlpha));
            }
            ds[i] = float(v);
            acc += v;
        }
        acc = wave_sum_f64(acc);
        if (lane == 0) {
            const double v = ps * base * (z_self > 0.0f ? 1.0 : double(kAlpha));
            ds_self[row] = float(v);
            dsq[row] = float(acc + v);
        }
    }
}

// ---- (c) the pooled edges and both plans --------------------------------------------------------------------------------------
struct PlanOut {
    int32_t* row_ptr;
    int32_t* col;
    int32_t* perm;
};

struct Params {
    const float* P;
    int64_t ldp;
    const int32_t* prp;
    int32_t B, K;
    int32_t n_cap_out, e_cap, sinks, sink_degree;
    int32_t m_rows;                    // n_cap_out - sinks: the rows that can be live
    int32_t row_tiles;                 // workgroups of the row fill section
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

// the live pooled rows, held to the capacities whatever the table says
__device__ __forceinline__ int32_t live_rows(const Params& p) { return p.K == 0 ? 0 : clampi(p.prp[p.B], 0, p.m_rows); }

// slot g's first pooled row and its row count m_g, held to [0, m_live] and to K
__device__ __forceinline__ int32_t slot_rows(const Params& p, int32_t g, int32_t m_live, int32_t& p0)
{
    p0 = clampi(p.prp[g], 0, m_live);
    return clampi(p.prp[g + 1] - p0, 0, min(p.K, m_live - p0));
}

// The mask of row c1 (< m_g) of slot g's block: bit c2 = "entry (c1, c2) is a pooled edge" — off the diagonal a non-zero entry
// below m_g, on it always.  Lanes at and beyond K load the row's last column (a clamped load, not a predicated one).
__device__ __forceinline__ uint64_t row_mask(const Params& p, int32_t g, int32_t c1, int32_t m_g, int lane)
{
    const int32_t c2 = min(lane, p.K - 1);
    const float v = p.P[(int64_t(g) * p.K + c1) * p.ldp + c2];
    return __ballot(lane < m_g && (lane == c1 || v != 0.0f));
}

__global__ void __launch_bounds__(kBlock) asap_count_kernel(const Params p)
{
    __shared__ int32_t wave_cnt[kWavesPerBlock];
    const int32_t g = int32_t(blockIdx.x);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int32_t p0;
    const int32_t m_g = slot_rows(p, g, live_rows(p), p0);             // workgroup-uniform
    int32_t cnt = 0;
    for (int32_t c1 = wave; c1 < m_g; c1 += kWavesPerBlock) cnt += __popcll(row_mask(p, g, c1, m_g, lane));
    if (lane == 0) wave_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t t = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) t += wave_cnt[w];
        p.slot_cnt[g] = t;
    }
}

// K == 0: no count launch ran, every slot is empty (count_valid == 0)
__global__ void __launch_bounds__(kScanBlock) asap_scan_kernel(const Params p, int32_t count_valid)
{
    const auto [begin, end] = thread_run(p.B);
    const int32_t kk = p.K * p.K;
    int64_t edges = 0;
    for (int32_t j = begin; j < end; ++j) edges += count_valid ? clampi(p.slot_cnt[j], 0, kk) : 0;
    int64_t edge_total;
    int64_t edge_run = block_exclusive_scan(edges, edge_total);
    for (int32_t j = begin; j < end; ++j) {
        p.slot_off[j] = int32_t(min(edge_run, int64_t(p.e_cap)));
        edge_run += count_valid ? clampi(p.slot_cnt[j], 0, kk) : 0;
    }
    if (threadIdx.x == 0) {
        const int32_t e_live = int32_t(min(edge_total, int64_t(p.e_cap)));
        p.slot_off[p.B] = e_live;
        p.counts[2] = e_live;
    }
}

// sections: [0, B) the slots; [B, B + row_tiles) the row_ptr of the dead and sink rows; behind them the padded tail
__global__ void __launch_bounds__(kBlock) asap_emit_kernel(const Params p)
{
    __shared__ uint64_t row_bits[kMaxK], col_bits[kMaxK];
    __shared__ int32_t row_off[kMaxK], col_off[kMaxK];
    const int32_t b = int32_t(blockIdx.x);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int32_t K = p.K;
    const int32_t m_live = live_rows(p);
    const int32_t e_live = clampi(p.slot_off[p.B], 0, p.e_cap);
    if (b < p.B) {
        int32_t p0;
        const int32_t m_g = slot_rows(p, b, m_live, p0);               // workgroup-uniform; rows [p0, p0 + m_g) are inside [0, m_live)
        if (m_g == 0) return;
        const int32_t e0 = clampi(p.slot_off[b], 0, e_live), e1 = clampi(p.slot_off[b + 1], e0, e_live);
        if (int32_t(threadIdx.x) < kMaxK) row_bits[threadIdx.x] = 0;
        __syncthreads();
        for (int32_t c1 = wave; c1 < m_g; c1 += kWavesPerBlock) {
            const uint64_t bits = row_mask(p, b, c1, m_g, lane);
            if (lane == 0) row_bits[c1] = bits;
        }
        __syncthreads();
        if (wave == 0) {
            // column `lane` of the bit matrix; the popcounts of row `lane` and column `lane`, scanned over the lanes
            uint64_t cb = 0;
            for (int32_t c1 = 0; c1 < m_g; ++c1) cb |= ((row_bits[c1] >> lane) & 1) << c1;      // a broadcast read
            const int32_t rc = __popcll(row_bits[lane]), cc = __popcll(cb);
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
        if (int32_t(threadIdx.x) < m_g) {
            const int32_t c = threadIdx.x, r = p0 + c;
            p.plan[0].row_ptr[r] = min(e0 + row_off[c], e1);
            p.plan[1].row_ptr[r] = min(e0 + col_off[c], e1);
        }
        for (int32_t c1 = wave; c1 < m_g; c1 += kWavesPerBlock) {
            const uint64_t rb = row_bits[c1];
            if (((rb >> lane) & 1) == 0) continue;
            const int32_t c2 = lane;
            const uint64_t off_diag = rb & ~(uint64_t(1) << c1);
            const bool loop = c2 == c1;
            const int32_t q = e0 + row_off[c1] + __popcll(loop ? off_diag : (off_diag & below(c2)));
            const int32_t qt = e0 + col_off[c2] + __popcll(col_bits[c2] & below(c1));
            if (q >= e1 || qt >= e1) continue;          // cannot happen while count and emit see the same P: held anyway
            p.out_row[q] = p0 + c1;
            p.out_col[q] = p0 + c2;
            p.out_src[q] = loop ? -1 : (b * K + c1) * K + c2;
            p.out_egi[q] = b;
            p.plan[0].col[q] = p0 + c2;
            p.plan[0].perm[q] = q;
            p.plan[1].col[qt] = p0 + c1;
            p.plan[1].perm[qt] = q;
        }
    } else if (b < p.B + p.row_tiles) {
        // row_ptr of rows [m_live, m_rows] is e_live, of row m_rows + t (t in [0, sinks]) the start of sink t: it holds the
        // padded edges [t, t + 1) * sink_degree of the tail.  (node_index and node_graph_index of these rows are the selection's.)
#pragma unroll
        for (int it = 0; it < kFillTile / kBlock; ++it) {
            const int64_t j = int64_t(b - p.B) * kFillTile + it * kBlock + threadIdx.x;
            if (j < m_live || j > p.n_cap_out) continue;
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

Workspace<2> edges_workspace(int64_t B) { return Workspace<2>{{4 * size_t(B > 0 ? B : 1), 4 * size_t(B + 1)}}; }

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

int check_max_k(const char* fn, int64_t K)
{
    if (K <= kMaxK) return TFGX_OK;
    set_error("%s: K = %lld is more than %d (TFGX_ASAPSTATIC_MAX_K)", fn, (long long)K, kMaxK);
    return TFGX_ERR_INVALID_ARG;
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_asapstatic_version(void) { return TFGX_ASAPSTATIC_ABI_VERSION; }

extern "C" int tfgx_asapstatic_attend_f32(const int32_t* row_ptr, const int32_t* col, int64_t N, int64_t E, const float* x,
                                          int64_t ldx, int64_t F, const float* sq, const float* sh, const float* bias,
                                          float drop_rate, uint64_t seed, const uint64_t* seed_dev, int32_t skip_self_loops,
                                          float* c, int64_t ldc, float* p, float* p_self, float* p_drop, float* p_self_drop,
                                          int32_t* bad_flag, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    const char* fn = "tfgx_asapstatic_attend_f32";
    const NamedSize sizes[] = {{"N", N}, {"E", E}, {"F", F}, {"N + E", N + E}};
    if (int rc = check_sizes(fn, sizes)) return rc;
    if (F > TFGX_ASAPSTATIC_MAX_FEATURES) return bad_arg(fn, "F exceeds TFGX_ASAPSTATIC_MAX_FEATURES", F);
    if (ldx < F) return bad_arg(fn, "ldx is smaller than F", ldx);
    if (ldc < F) return bad_arg(fn, "ldc is smaller than F", ldc);
    if (!(drop_rate >= 0.0f && drop_rate < 1.0f)) {
        set_error("%s: drop_rate = %g must be in [0, 1)", fn, double(drop_rate));
        return TFGX_ERR_INVALID_ARG;
    }
    if (N == 0) return TFGX_OK;
    const char* bad = nullptr;
    if (row_ptr == nullptr) bad = "row_ptr";
    else if (col == nullptr && E > 0) bad = "col";
    else if (x == nullptr && F > 0) bad = "x";
    else if (c == nullptr && F > 0) bad = "c";
    else if (sq == nullptr) bad = "sq";
    else if (sh == nullptr) bad = "sh";
    else if (bias == nullptr) bad = "bias";
    else if (p == nullptr && E > 0) bad = "p";
    else if (p_self == nullptr) bad = "p_self";
    else if (drop_rate > 0.0f && p_drop == nullptr && E > 0) bad = "p_drop";
    else if (drop_rate > 0.0f && p_self_drop == nullptr) bad = "p_self_drop";
    if (bad != nullptr) return null_arg(fn, bad);
    hipStream_t stream = as_stream(stream_);
    const DropCfg drop = make_drop(drop_rate, seed, E, seed_dev);
    if (skip_self_loops != 0)
        asap_attend::launch<true>(row_ptr, col, N, E, x, ldx, F, sq, sh, bias, drop, c, ldc, p, p_self, p_drop, p_self_drop,
                                  bad_flag, stream);
    else
        asap_attend::launch<false>(row_ptr, col, N, E, x, ldx, F, sq, sh, bias, drop, c, ldc, p, p_self, p_drop, p_self_drop,
                                   bad_flag, stream);
    TFGX_LAUNCH_CHECK("asap_attend::kernel");
    return TFGX_OK;
}

extern "C" int tfgx_asapstatic_attend_backward_f32(const int32_t* row_ptr, const int32_t* col, int64_t N, int64_t E, const float* sq,
                                                   const float* sh, const float* bias, const float* p, const float* p_self,
                                                   const float* p_drop, const float* p_self_drop, const float* dp,
                                                   const float* dp_self, int32_t skip_self_loops, float* ds, float* ds_self,
                                                   float* dsq, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    const char* fn = "tfgx_asapstatic_attend_backward_f32";
    const NamedSize sizes[] = {{"N", N}, {"E", E}, {"N + E", N + E}};
    if (int rc = check_sizes(fn, sizes)) return rc;
    if (N == 0) return TFGX_OK;
    const char* bad = nullptr;
    if (row_ptr == nullptr) bad = "row_ptr";
    else if (col == nullptr && E > 0) bad = "col";
    else if (sq == nullptr) bad = "sq";
    else if (sh == nullptr) bad = "sh";
    else if (bias == nullptr) bad = "bias";
    else if (p == nullptr && E > 0) bad = "p";
    else if (p_self == nullptr) bad = "p_self";
    else if (dp == nullptr && E > 0) bad = "dp";
    else if (dp_self == nullptr) bad = "dp_self";
    else if (ds == nullptr && E > 0) bad = "ds";
    else if (ds_self == nullptr) bad = "ds_self";
    else if (dsq == nullptr) bad = "dsq";
    if (bad != nullptr) return null_arg(fn, bad);
    // dropout was applied <=> p_self_drop is given (every row has a self edge); p_drop goes with it wherever there are edges
    if ((E > 0 && (p_drop == nullptr) != (p_self_drop == nullptr)) || (E == 0 && p_drop != nullptr && p_self_drop == nullptr)) {
        set_error("%s: give both p_drop and p_self_drop, or neither", fn);
        return TFGX_ERR_INVALID_ARG;
    }
    asap_attend_backward_centred_kernel<<<grid_for(N, kWavesPerBlock), kBlock, 0, as_stream(stream_)>>>(
        row_ptr, col, N, E, sq, sh, bias, p, p_self, p_drop != nullptr ? p_drop : p, p_self_drop != nullptr ? p_self_drop : p_self,
        dp, dp_self, p_self_drop != nullptr ? 1 : 0, skip_self_loops, ds, ds_self, dsq);
    TFGX_LAUNCH_CHECK("asap_attend_backward_centred_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_asapstatic_assign_f32(const int32_t* row_ptr, const int32_t* col, int64_t N, int64_t E, const float* p,
                                          const float* p_self, int32_t skip_self_loops, const int32_t* node_index,
                                          const int32_t* pooled_node_graph_index, const int32_t* pooled_row_ptr, int64_t B,
                                          int64_t m_rows, int64_t K, float* S, int64_t lds, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    const char* fn = "tfgx_asapstatic_assign_f32";
    const NamedSize sizes[] = {{"N", N}, {"E", E}, {"B", B}, {"m_rows", m_rows}, {"K", K}, {"lds", lds}};
    if (int rc = check_sizes(fn, sizes)) return rc;
    if (int rc = check_max_k(fn, K)) return rc;
    if (lds < K) return bad_arg(fn, "lds is smaller than K", lds);
    if (N == 0 || K == 0) return TFGX_OK;
    const char* bad = nullptr;
    if (S == nullptr) bad = "S";
    else if (m_rows == 0) bad = nullptr;                  // nothing but S is read
    else if (row_ptr == nullptr) bad = "row_ptr";
    else if (col == nullptr && E > 0) bad = "col";
    else if (p == nullptr && E > 0) bad = "p";
    else if (p_self == nullptr) bad = "p_self";
    else if (node_index == nullptr) bad = "node_index";
    else if (pooled_node_graph_index == nullptr) bad = "pooled_node_graph_index";
    else if (pooled_row_ptr == nullptr) bad = "pooled_row_ptr";
    if (bad != nullptr) return null_arg(fn, bad);
    hipStream_t stream = as_stream(stream_);
    asap_zero_kernel<<<grid_for(N * K, kBlock), kBlock, 0, stream>>>(S, N * K, K, lds);
    TFGX_LAUNCH_CHECK("asap_zero_kernel");
    if (m_rows == 0) return TFGX_OK;
    const int64_t grid = (m_rows + kWavesPerBlock - 1) / kWavesPerBlock;      // below 2^29
    asap_assign_kernel<<<static_cast<unsigned>(grid), kBlock, 0, stream>>>(row_ptr, col, int32_t(N), int32_t(E), p, p_self,
                                                                           skip_self_loops, node_index, pooled_node_graph_index,
                                                                           pooled_row_ptr, int32_t(B), int32_t(m_rows), int32_t(K),
                                                                           S, lds);
    TFGX_LAUNCH_CHECK("asap_assign_kernel");
    return TFGX_OK;
}

extern "C" size_t tfgx_asapstatic_edges_workspace_bytes(int64_t B)
{
    if (B < 0 || B > TFGX_ASAPSTATIC_MAX_SLOTS) return 0;
    return edges_workspace(B).bytes();
}

extern "C" int tfgx_asapstatic_edges(const tfgx_asapstatic_edges_args* a, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    const char* fn = "tfgx_asapstatic_edges";
    if (a == nullptr) return null_arg(fn, "args");
    const NamedSize sizes[] = {{"B", a->B}, {"K", a->K}, {"ldp", a->ldp}, {"n_cap_out", a->n_cap_out}, {"e_cap", a->e_cap},
                               {"sinks", a->sinks}, {"sink_degree", a->sink_degree}};
    if (int rc = check_sizes(fn, sizes)) return rc;
    if (a->B > TFGX_ASAPSTATIC_MAX_SLOTS) {
        set_error("%s: B = %lld is more than the %d slots one workgroup scans", fn, (long long)a->B, TFGX_ASAPSTATIC_MAX_SLOTS);
        return TFGX_ERR_INVALID_ARG;
    }
    if (int rc = check_max_k(fn, a->K)) return rc;
    if (a->ldp < a->K) return bad_arg(fn, "ldp is smaller than K", a->ldp);
    if (int rc = check_sink_degree(fn, a->sink_degree)) return rc;
    if (int rc = check_sinks_within(fn, a->sinks, "n_cap_out", a->n_cap_out)) return rc;
    if (int rc = check_sink_tail(fn, a->sinks, a->sink_degree, a->e_cap)) return rc;
    if (int rc = check_size(fn, "B * K * K", a->B * a->K * a->K)) return rc;      // B K below 2^26
    const int64_t most = a->K * (a->n_cap_out - a->sinks);                        // below 2^37
    if (a->e_cap < most) {
        set_error("%s: e_cap = %lld is smaller than K * (n_cap_out - sinks) = %lld", fn, (long long)a->e_cap, (long long)most);
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
    else if (a->pooled_row_ptr == nullptr) bad = "pooled_row_ptr";
    else if (a->workspace == nullptr) bad = "workspace";
    else if (a->B > 0 && a->K > 0 && a->P == nullptr) bad = "P";
    else if (a->e_cap > 0 && a->out_row == nullptr) bad = "out_row";
    else if (a->e_cap > 0 && a->out_col == nullptr) bad = "out_col";
    else if (a->e_cap > 0 && a->out_edge_src == nullptr) bad = "out_edge_src";
    else if (a->e_cap > 0 && a->out_edge_graph_index == nullptr) bad = "out_edge_graph_index";
    if (bad != nullptr) return null_arg(fn, bad);
    const Workspace<2> ws = edges_workspace(a->B);
    if (a->workspace_bytes < ws.bytes()) {
        set_error("%s: workspace_bytes = %zu is smaller than the %zu bytes tfgx_asapstatic_edges_workspace_bytes asks for", fn,
                  a->workspace_bytes, ws.bytes());
        return TFGX_ERR_WORKSPACE;
    }

    Params p = {};
    p.P = a->P, p.ldp = a->ldp, p.prp = a->pooled_row_ptr;
    p.B = int32_t(a->B), p.K = int32_t(a->K);
    p.n_cap_out = int32_t(a->n_cap_out), p.e_cap = int32_t(a->e_cap), p.sinks = int32_t(a->sinks);
    p.sink_degree = int32_t(a->sink_degree);
    p.m_rows = int32_t(a->n_cap_out - a->sinks);
    p.row_tiles = int32_t((a->n_cap_out + 1 + kFillTile - 1) / kFillTile);
    p.out_row = a->out_row, p.out_col = a->out_col, p.out_src = a->out_edge_src, p.out_egi = a->out_edge_graph_index;
    p.plan[0] = PlanOut{a->plan->out_row_ptr, a->plan->out_col, a->plan->out_perm};
    p.plan[1] = PlanOut{a->plan_t->out_row_ptr, a->plan_t->out_col, a->plan_t->out_perm};
    p.counts = a->counts;
    p.slot_cnt = ws.at<int32_t>(a->workspace, 0);
    p.slot_off = ws.at<int32_t>(a->workspace, 1);

    const bool slots = p.B > 0 && p.K > 0;
    if (slots) {
        asap_count_kernel<<<static_cast<unsigned>(p.B), kBlock, 0, stream>>>(p);
        TFGX_LAUNCH_CHECK("asap_count_kernel");
    }
    asap_scan_kernel<<<1, kScanBlock, 0, stream>>>(p, slots ? 1 : 0);
    TFGX_LAUNCH_CHECK("asap_scan_kernel");
    const int64_t edge_tiles = (a->e_cap + kFillTile - 1) / kFillTile;
    const int64_t grid = int64_t(p.B) + p.row_tiles + edge_tiles;      // each term is below 2^31 / 1024 or 2^20
    asap_emit_kernel<<<static_cast<unsigned>(grid), kBlock, 0, stream>>>(p);
    TFGX_LAUNCH_CHECK("asap_emit_kernel");
    return TFGX_OK;
}
