// Aggregation -> projection in ONE launch:  C = act( (reduce_{edges of r} w * x[col] (+ self_coef[r] * x[r]) [/ deg]) @ B + bias )
// for the aggregate-then-project layers — GCN when units > F (nn/conv/gcn.py:272-288 evaluated as (A_hat x) W), mean / sum
// GraphSAGE's neighbour half (nn/conv/graph_sage.py:34-58) — instead of tfgx_segment_reduce_f32 writing the [N, F] aggregate
// to HBM and tfgx_gemm_bias_act_f32 reading it back (1.9 GB of round trip at products shape, F = 100).
//
// One persistent 1024-thread workgroup per CU (16 waves; the gather walk keeps its rate down to 16 waves per CU:
// profiles/r03_occupancy_probe.jsonl).  LDS holds B ([KP][LDW] floats, loaded once) and two tiles of aggregated
// rows, TRANSPOSED (At[k][m], m = destination row inside the 64-row tile) so that the MFMA A operand is a conflict-free
// ds_read over consecutive m.  When all of B does not fit beside the two tiles (F = 128 -> 256: 135 KB + 66 KB > 160 KB)
// only its first NL columns (a multiple of 64) are resident; the consumer jobs of the remaining columns read their B
// operand straight from global memory — 128-byte row segments of a <= 128 KB matrix that every workgroup re-reads for every
// tile, i.e. L2 hits — with 8 k-pairs (16 loads) in flight per wave.
//   * producers: every wave repeatedly takes the next UNIT (64 / G consecutive destination rows of the current tile: one per
//     lane group) from an LDS counter, reduces it exactly like seg_reduce_kernel (G lanes per row, 4 columns per lane,
//     (col, w) batches prefetched, 8 gathered rows in flight, one in-order FMA chain per output element), and stores the row
//     into the tile.  Units are handed out dynamically, so a wave that drew short rows simply takes more of them;
//   * consumers: the last waves to arrive at a tile (per-tile arrival counter) each multiply one 32-row x 64-column block of
//     it — v_mfma_f32_32x32x2_f32 against B from LDS, bias / activation in the epilogue, rows written straight to C — while
//     the other waves are already reducing the next tile into the other buffer.  No workgroup barrier after the B load: a
//     buffer is re-used only after its `done` sequence number says the previous occupant has been multiplied.
// Deterministic (fixed per-row edge order, fixed k order), fp32 throughout.  Roofline: HBM (the gather), as the unfused
// aggregation; the MFMA work (2 N F U flops = 0.8 ms of one wave per CU at products shape) rides on otherwise idle pipes.
#include "tfgx_fused_common.h"

namespace tfgx {
namespace {

struct FArgs : FusedProj {
    const int32_t* row_ptr;
    const int32_t* col;
    const float* w;
    const float* x;
    int64_t ldx;
    int32_t op;
    const float* self_coef;
    const int32_t* mean_count;
    float* agg;        // optional side output (training forward): the aggregated rows themselves, [n_dst, ld_agg], or NULL
    int64_t ld_agg;
    // power-law graphs: rows longer than hub_threshold were cut into chunks and reduced chunk by chunk into hub_scratch by a
    // launch of the ordinary kernel BEFORE this one; their lane group folds the chunk partials in chunk order instead of
    // walking the edges (what hub_finalize_kernel does in the unfused path)
    int32_t hub_threshold;
    int32_t n_hub;
    const int32_t* hub_rows;        // ascending
    const int32_t* hub_chunk_ptr;
    const float* hub_scratch;       // [chunks, F]
    const int32_t* hub_order_slot;  // optional: slot of row row_order[i] in hub_rows, i < n_hub (rows sorted by length: hubs first)
    // optional split source rows (the static feature layout, tfgx_reduce_args.x_tail / edge_tail): x holds columns [0, f_main),
    // x_tail columns [f_main, F) per NODE, edge_tail the same tail columns per EDGE of this plan (streamed next to col / w)
    const float* x_tail;
    int64_t ld_tail;
    int32_t f_main;
    const float* edge_tail;
    int64_t ld_edge_tail;
};

template <int G, bool WEIGHTED>
__global__ __launch_bounds__(kFusedThreads) void agg_gemm_kernel(const FArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const FusedLds sh = fused_lds_init(a, lds);
    constexpr int RPW = 64 / G;                             // destination rows per wave step (one per lane group)
    constexpr int UNITS = kTileRows / RPW;
    constexpr int UNROLL = 8;
    const int tid = threadIdx.x, lane64 = tid & 63;
    const int lane = lane64 % G, grp = lane64 / G;

    const int64_t my_tiles = a.n_tiles > int64_t(blockIdx.x) ? (a.n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    const int64_t total_units = my_tiles * UNITS;
    const int c_raw = lane * 4;
    const bool cvalid = c_raw < a.F;
    const int coff = cvalid ? c_raw : a.F - 4;              // lanes past F re-read the last valid vector (discarded)
    // per-lane source base / stride (seg_reduce_kernel's SPLIT scheme): one array normally; with split rows the lanes that own
    // columns >= f_main read the node-tail array — or, for gathered rows, the per-EDGE tail stream (indexed by CSR position)
    const float* xb = a.x + coff;           // gathered rows
    int64_t xl = a.ldx;
    const float* xsb = xb;                  // a NODE's own row (the self-loop term)
    int64_t xsl = xl;
    bool by_edge = false;
    if (a.x_tail != nullptr && coff >= a.f_main) {
        xb = xsb = a.x_tail + (coff - a.f_main);
        xl = xsl = a.ld_tail;
        if (a.edge_tail != nullptr) {
            xb = a.edge_tail + (coff - a.f_main);
            xl = a.ld_edge_tail;
            by_edge = true;
        }
    }
    // element offset of a gathered row as ONE 32 x 32 -> 64-bit multiply (v_mad_u64_u32): ids / CSR positions are non-negative
    // int32 and the strides fit 32 bits (checked at the entry point); int64 x int64 is emulated with three quarter-rate
    // multiplies per address — vector-ALU work the MFMA half of this kernel competes with
    const uint32_t xl32 = uint32_t(xl);
    auto row_off = [&](int i) { return uint64_t(uint32_t(i)) * xl32; };

    while (true) {
        int u = 0;
        if (lane64 == 0) u = atomicAdd(&sh.ctrl[0], 1);
        u = __builtin_amdgcn_readfirstlane(u);
        if (u >= total_units) break;
        const int q = u / UNITS, slot = u - q * UNITS;      // tile sequence number inside this workgroup, unit inside the tile
        const int buf = q % kBufs;
        const int64_t tile = int64_t(blockIdx.x) + int64_t(q) * gridDim.x;
        const int m = slot * RPW + grp;                     // row inside the tile
        const int64_t ri = tile * kTileRows + m;
        const int64_t r = (a.row_order != nullptr && ri < a.n_dst) ? int64_t(a.row_order[ri]) : ri;

        // ---- producer: reduce destination row r (seg_reduce_kernel's walk) -------------------------------------------
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
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
                // chunk partials in chunk order, eight loads in flight (thousands of chunks on the longest rows)
                int c = a.hub_chunk_ptr[lo];
                const int c_end = a.hub_chunk_ptr[lo + 1];
                for (; c + UNROLL <= c_end; c += UNROLL) {
                    float pv[UNROLL][4];
#pragma unroll
                    for (int t = 0; t < UNROLL; ++t) load_vec<4>(a.hub_scratch + int64_t(c + t) * a.F + coff, pv[t]);
#pragma unroll
                    for (int t = 0; t < UNROLL; ++t)
#pragma unroll
                        for (int v = 0; v < 4; ++v) acc[v] += pv[t][v];
                }
                for (; c < c_end; ++c) {
                    float pv[4];
                    load_vec<4>(a.hub_scratch + int64_t(c) * a.F + coff, pv);
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[v] += pv[v];
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
                int j = 0;
                for (; j + UNROLL <= cnt; j += UNROLL) {
                    float xv[UNROLL][4];
                    float ww[UNROLL];
#pragma unroll
                    for (int t = 0; t < UNROLL; ++t) {
                        const int c = bcast_i<G>(cj, j + t);
                        if constexpr (WEIGHTED) ww[t] = bcast_f<G>(wj, j + t);
                        load_vec<4>(xb + row_off(by_edge ? base + j + t : c), xv[t]);
                    }
#pragma unroll
                    for (int t = 0; t < UNROLL; ++t)
#pragma unroll
                        for (int v = 0; v < 4; ++v) acc[v] = WEIGHTED ? fmaf(ww[t], xv[t][v], acc[v]) : acc[v] + xv[t][v];
                }
                for (; j < cnt; ++j) {
                    const int c = bcast_i<G>(cj, j);
                    float wv = 1.0f;
                    if constexpr (WEIGHTED) wv = bcast_f<G>(wj, j);
                    float xv[4];
                    load_vec<4>(xb + row_off(by_edge ? base + j : c), xv);
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[v] = WEIGHTED ? fmaf(wv, xv[v], acc[v]) : acc[v] + xv[v];
                }
            }
            if (a.self_coef) {                               // the implicit (r, r) edge appended after the row's edges
                const float sc = a.self_coef[r];
                float xs[4];
                load_vec<4>(xsb + r * xsl, xs);
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[v] = fmaf(sc, xs[v], acc[v]);
            }
            if (a.op == TFGX_MEAN) {
                const int cnt = a.mean_count ? a.mean_count[r] : (e - s);
                const float divisor = float(cnt > 1 ? cnt : 1);
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[v] = acc[v] / divisor;
            }
        }
        if (a.agg != nullptr && cvalid && r < a.n_dst)        // training forward: the weight gradient needs the aggregate
            store_vec<4>(a.agg + r * a.ld_agg + coff, acc);
        // ---- hand the row over: wait until the buffer's previous tile has been multiplied, store transposed ----------------
        fused_wait_buffer(sh, q, buf);
        float* ab = sh.At + buf * a.KP * kLda;
        if (cvalid) {
#pragma unroll
            for (int v = 0; v < 4; ++v) ab[(coff + v) * kLda + m] = acc[v];
        }
        if (a.row_order != nullptr && lane == 0) sh.rowid[buf * kTileRows + m] = ri < a.n_dst ? int(r) : -1;
        fused_arrive_and_multiply<UNITS>(a, sh, q, buf, tile, lane64);
    }
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

// 1 if tfgx_aggregate_gemm_f32 takes rows of F columns projected to N columns: the two tiles and at least 64 columns of B
// resident in 160 KB of LDS (columns that do not fit are read from global memory / L2 by their consumer jobs)
extern "C" int tfgx_aggregate_gemm_fits(int64_t F, int64_t N)
{
    if (F < 4 || F > 128 || F % 4 != 0 || N < 1 || N > 256) return 0;
    const int kp = int((F + 1) / 2 * 2), np = int((N + 127) / 128) * 128;
    return fused_resident_cols(kp, np) > 0 ? 1 : 0;
}

extern "C" int tfgx_aggregate_gemm_f32(const tfgx_reduce_args* p, const float* B, int64_t ldb, const float* bias, int32_t act,
                                       float* C, int64_t ldc, int64_t N, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    TFGX_REQUIRE(p != nullptr, "args is null");
    TFGX_REQUIRE(p->op == TFGX_SUM || p->op == TFGX_MEAN, "sum / mean only");
    TFGX_REQUIRE(act == TFGX_ACT_NONE || act == TFGX_ACT_RELU, "bad act");
    TFGX_REQUIRE(tfgx_aggregate_gemm_fits(p->F, N) == 1, "shape not supported (tfgx_aggregate_gemm_fits)");
    TFGX_REQUIRE(p->n_dst >= 0 && p->n_dst < (int64_t(1) << 31) * kTileRows / 64, "bad n_dst");
    if (p->n_dst == 0) return TFGX_OK;
    TFGX_REQUIRE(p->row_begin && p->row_end == p->row_begin + 1 && p->rp_stride == 1, "needs a plain CSR (row_ptr, row_ptr + 1)");
    TFGX_REQUIRE(p->x && B && C, "null pointer");          // (col may be NULL for a graph without edges)
    TFGX_REQUIRE(p->ldx >= (p->x_tail ? p->f_main : p->F) && p->ldx % 4 == 0 && aligned_to(p->x, 16) && ldb >= N && ldc >= N,
                 "bad leading dimension / alignment");
    TFGX_REQUIRE(!p->accumulate && !p->add_x && !p->track, "plain aggregation only (no accumulate / add_x / track)");
    TFGX_REQUIRE(p->ldx < (int64_t(1) << 31) && p->ld_tail < (int64_t(1) << 31) && p->ld_edge_tail < (int64_t(1) << 31),
                 "leading dimensions must be below 2^31 elements");
    if (p->x_tail) {      // split source rows (static feature layout): whole-line main rows + 16-byte aligned tails
        TFGX_REQUIRE(p->f_main >= 4 && p->f_main % 4 == 0 && p->f_main < p->F && p->ldx >= p->f_main && p->ld_tail >= p->F - p->f_main &&
                         p->ld_tail % 4 == 0 && aligned_to(p->x_tail, 16),
                     "split rows: bad f_main / ld_tail / alignment");
        TFGX_REQUIRE(p->edge_tail == nullptr || (p->ld_edge_tail >= p->F - p->f_main && p->ld_edge_tail % 4 == 0 &&
                                                 aligned_to(p->edge_tail, 16)),
                     "split rows: bad edge_tail stride / alignment");
    }
    TFGX_REQUIRE(p->out == nullptr || (p->ldo >= p->F && p->ldo % 4 == 0 && aligned_to(p->out, 16)),
                 "side output of the aggregate: rows of >= F floats, 16-byte aligned");
    const bool use_hub = p->hub_threshold > 0 && p->n_hub_rows > 0;
    if (use_hub) {
        TFGX_REQUIRE(p->hub_rows && p->hub_chunk_ptr && p->hub_chunk_begin && p->hub_chunk_end && p->hub_scratch &&
                         p->n_hub_chunks > 0 && p->n_hub_rows < (int64_t(1) << 31),
                     "hub rows given without chunk lists / scratch");
        // chunk partials first: every chunk is reduced like an ordinary row into hub_scratch (the unfused path's step 2)
        const tfgx_reduce_args c = fused_hub_chunk_args(p);
        const int rc = tfgx_segment_reduce_f32(&c, stream_);
        if (rc != TFGX_OK) return rc;
    }
    FArgs a;
    a.hub_threshold = use_hub ? p->hub_threshold : 0;
    a.n_hub = use_hub ? int32_t(p->n_hub_rows) : 0;
    a.hub_rows = p->hub_rows; a.hub_chunk_ptr = p->hub_chunk_ptr; a.hub_scratch = p->hub_scratch;
    a.row_ptr = p->row_begin; a.col = p->col; a.w = p->w; a.x = p->x; a.ldx = p->ldx;
    a.op = p->op; a.self_coef = p->self_coef; a.mean_count = p->mean_count;
    fused_fill_proj(a, p, B, ldb, bias, act, C, ldc, N);
    a.hub_order_slot = use_hub ? p->hub_order_slot : nullptr;
    a.x_tail = p->x_tail; a.ld_tail = p->ld_tail; a.f_main = int32_t(p->x_tail ? p->f_main : p->F);
    a.edge_tail = p->x_tail ? p->edge_tail : nullptr; a.ld_edge_tail = p->ld_edge_tail;
    a.agg = p->out; a.ld_agg = p->ldo;
    hipStream_t stream = as_stream(stream_);
    const bool weighted = p->w != nullptr;
    if (p->F <= 64) {
        return weighted ? fused_launch<agg_gemm_kernel<16, true>>(__func__, "agg_gemm_kernel", a, stream)
                        : fused_launch<agg_gemm_kernel<16, false>>(__func__, "agg_gemm_kernel", a, stream);
    }
    return weighted ? fused_launch<agg_gemm_kernel<32, true>>(__func__, "agg_gemm_kernel", a, stream)
                    : fused_launch<agg_gemm_kernel<32, false>>(__func__, "agg_gemm_kernel", a, stream);
}
