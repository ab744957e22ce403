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
// The LDS set-up, the consumer (hand-over, MFMA loops, epilogue, stores) and the host side of the launch are shared with
// tfgx_fused.hip: tfgx_fused_common.h.
#include "tfgx_fused_common.h"
#include "../../include/tfgx_fused_h16.h"
#include <cstdio>
#include <cstring>
#include <type_traits>

namespace tfgx {
namespace {

constexpr int kVec = 8;      // elements per 16-byte vector of a 16-bit table

struct FHArgs : FusedProj {
    const int32_t* row_ptr;
    const int32_t* col;
    const float* w;
    const uint16_t* x;      // [n_src, ldx] 16-bit elements
    int64_t ldx;
    int32_t op;
    const float* self_coef;
    const int32_t* mean_count;
    float* agg;        // optional side output: the aggregated rows themselves, [n_dst, ld_agg] fp32, or NULL
    int64_t ld_agg;
    int32_t hub_threshold;
    int32_t n_hub;
    const int32_t* hub_rows;        // ascending
    const int32_t* hub_chunk_ptr;
    const float* hub_scratch;       // [chunks, F] fp32 chunk partials (written by tfgx_segment_reduce_h16 before this launch)
    const int32_t* hub_order_slot;
};

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
    const FusedLds sh = fused_lds_init(a, lds);
    constexpr int RPW = 64 / G;                             // destination rows per wave step (one per lane group)
    constexpr int UNITS = kTileRows / RPW;
    constexpr int UNROLL = 8;
    static_assert(G == 8 || G == 16, "UNITS = G must cover the eight consumer jobs of a tile");
    const int tid = threadIdx.x, lane64 = tid & 63;
    const int lane = lane64 % G, grp = lane64 / G;

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
    const uint16_t* xb = a.x + coff;
    // element offset of a gathered row as ONE 32 x 32 -> 64-bit multiply: ids are non-negative int32, the stride fits 32 bits
    const uint32_t xl32 = uint32_t(a.ldx);
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
        // ---- hand the row over: wait until the buffer's previous tile has been multiplied, store transposed ----------------
        fused_wait_buffer(sh, q, buf);
        float* ab = sh.At + buf * a.KP * kLda;
        if (v_lo) {
#pragma unroll
            for (int v = 0; v < 4; ++v) ab[(c0 + v) * kLda + m] = acc[v];
        }
        if (v_hi) {
#pragma unroll
            for (int v = 4; v < kVec; ++v) ab[(c0 + v) * kLda + m] = acc[v];
        }
        if (a.row_order != nullptr && lane == 0) sh.rowid[buf * kTileRows + m] = ri < a.n_dst ? int(r) : -1;
        fused_arrive_and_multiply<UNITS>(a, sh, q, buf, tile, lane64);
    }
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

template <int DT>
int launch_dt(const char* fn, const FHArgs& a, int g, bool weighted, hipStream_t stream)
{
    const char* name = "agg_gemm_h16_kernel";
    if (g == 8) return weighted ? fused_launch<agg_gemm_h16_kernel<DT, 8, true>>(fn, name, a, stream)
                                : fused_launch<agg_gemm_h16_kernel<DT, 8, false>>(fn, name, a, stream);
    return weighted ? fused_launch<agg_gemm_h16_kernel<DT, 16, true>>(fn, name, a, stream)
                    : fused_launch<agg_gemm_h16_kernel<DT, 16, false>>(fn, name, a, stream);
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
        const tfgx_reduce_args c = fused_hub_chunk_args(p);
        const int rc = tfgx_segment_reduce_h16(&c, x_dtype, TFGX_DT_F32, stream_);
        if (rc != TFGX_OK) return rc;
    }
    FHArgs a;
    a.hub_threshold = use_hub ? p->hub_threshold : 0;
    a.n_hub = use_hub ? int32_t(p->n_hub_rows) : 0;
    a.hub_rows = p->hub_rows; a.hub_chunk_ptr = p->hub_chunk_ptr; a.hub_scratch = p->hub_scratch;
    a.hub_order_slot = use_hub ? p->hub_order_slot : nullptr;
    a.row_ptr = p->row_begin; a.col = p->col; a.w = p->w;
    a.x = static_cast<const uint16_t*>(static_cast<const void*>(p->x)); a.ldx = p->ldx;
    a.op = p->op; a.self_coef = p->self_coef; a.mean_count = p->mean_count;
    fused_fill_proj(a, p, B, ldb, bias, act, C, ldc, N);
    a.agg = static_cast<float*>(p->out); a.ld_agg = p->ldo;
    hipStream_t stream = as_stream(stream_);
    const bool weighted = p->w != nullptr;
    const int g = group_lanes(p->F);
    if (x_dtype == TFGX_DT_BF16) return launch_dt<TFGX_DT_BF16>(__func__, a, g, weighted, stream);
    return launch_dt<TFGX_DT_F16>(__func__, a, g, weighted, stream);
}
