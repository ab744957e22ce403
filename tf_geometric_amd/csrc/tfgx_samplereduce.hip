// The fused input hop (include/tfgx_samplereduce.h): draw the neighbours of every listed node and reduce their feature rows in
// ONE launch.  The drawn (id, weight) pairs never leave the chip.
//
// Reference: tf_geometric/utils/graph_utils.py:630-772 (RandomNeighborSampler), demo/demo_graph_sage.py.
//
// A wave owns a tile of up to 64 listed rows and 1024 LDS slots; row l of the tile keeps its list in slots [l * k, l * k + m).
//   phase 1, draw  : lane l runs sample_row_lane for row l of the tile (the body tfgx_nbrblock_sample_rows runs, the LDS slots as
//                    its output); the rows sample_row_is_long names are then taken one by one by the whole wave
//                    (sample_row_wave).  Same bodies, same (seed, row id) key: the same ids and weights, bit for bit.
//   phase 2, reduce: the wave is cut into 64 / G groups of G lanes, a group per row, a lane per (chunk of) column(s); every
//                    lane walks its row's list in draw order with kInFlight row loads in flight.  Lanes past the list or past the last
//                    column load a CLAMPED address and drop the value with a select: no load is predicated.
// Nothing is passed between waves; the two phases of a tile are ordered by a wave-level fence (LDS executes one wave's
// instructions in order).
#include "tfgx_common.h"
#include "tfgx_host.h"
#include "tfgx_sample_rows.h"
#include "tfgx_widen_h16.h"
#include "../../include/tfgx_samplereduce.h"
#include "../../include/tfgx_nbrstatic.h"
#include "../../include/tfgx_minibatch_h16.h"

namespace tfgx {
namespace {

#define TFGX_STR_(v) #v
#define TFGX_STR(v) TFGX_STR_(v)

constexpr int kSlots = 4 * TFGX_SAMPLEREDUCE_MAX_DRAWS;      // (id, weight) pairs a wave keeps: 8 KiB
constexpr int kWaves = kBlock / kWave;
constexpr int kInFlight = 4;                                 // row loads in flight per lane
static_assert(TFGX_SAMPLEREDUCE_MAX_DRAWS >= 128 && kSlots >= TFGX_SAMPLEREDUCE_MAX_DRAWS, "every branch of both bodies must be reachable");

// orders this wave's LDS writes before its later LDS reads (and the reverse): a compiler fence, the hardware keeps the order
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int wave_max(int v)
{
    for (int off = kWave / 2; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return __builtin_amdgcn_readfirstlane(v);
}

// the element a table of type DT stores: a float, or the raw 16 bits of a bf16 / fp16 (include/tfgx_h16.h)
template <int DT> struct ElemOf { using type = uint16_t; };
template <> struct ElemOf<TFGX_DT_F32> { using type = float; };

// columns [col0, col0 + ncols * VEC) of the n_tile rows of a tile; G = 1 << lg lanes per row.  `m` / `ok` are lane l's values
// for row l of the tile.  A 16-bit table (DT != TFGX_DT_F32) is read in chunks of VEC = 8 elements, one 16-byte load each, widened
// in registers; its last chunk may reach past column `f_end` into the row's pad columns, which are accumulated and never stored.
template <int DT, int VEC>
__device__ __forceinline__ void reduce_tile(const int32_t* s_col, const float* s_w, int k, int n_tile, int64_t base, int m,
                                            int ok, const typename ElemOf<DT>::type* __restrict__ x, int64_t ldx, int col0,
                                            int ncols, int f_end, int lg, int op, float* __restrict__ out, int64_t ldo,
                                            bool out_vec, int lane)
{
    constexpr bool kHalf = DT != TFGX_DT_F32;
    static_assert(!kHalf || VEC == kVec, "a 16-bit table is read in 16-byte vectors");
    const int G = 1 << lg, R = kWave >> lg;
    const int sub = lane >> lg, cl = lane & (G - 1);
    for (int l0 = 0; l0 < n_tile; l0 += R) {
        const int l = l0 + sub;
        const bool live = l < n_tile;
        const int ls = live ? l : n_tile - 1;
        const int m_any = __shfl(m, ls), ok_l = __shfl(ok, ls);
        const int m_l = live ? m_any : 0;
        const int m_max = wave_max(m_l);
        const int o = ls * k, last = max(m_l - 1, 0);
        for (int c0 = 0; c0 < ncols; c0 += G) {
            const int c = c0 + cl;
            const typename ElemOf<DT>::type* xc = x + col0 + int64_t(min(c, ncols - 1)) * VEC;
            float acc[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = 0.0f;
            for (int j0 = 0; j0 < m_max; j0 += kInFlight) {
                int32_t id[kInFlight];
                float wt[kInFlight], v[kInFlight][VEC];
#pragma unroll
                for (int u = 0; u < kInFlight; ++u) {
                    const int p = o + min(j0 + u, last);             // past the list: its last slot again (an empty row's
                    id[u] = s_col[p];                                // first slot holds id 0), dropped below
                    wt[u] = s_w[p];
                }
                // every load is issued whatever its lane keeps of it: the values are opaque until all of them are in flight
                if constexpr (kHalf) {
                    uint4 raw[kInFlight];
#pragma unroll
                    for (int u = 0; u < kInFlight; ++u) raw[u] = *reinterpret_cast<const uint4*>(xc + int64_t(id[u]) * ldx);
#pragma unroll
                    for (int u = 0; u < kInFlight; ++u) asm volatile("" : "+v"(raw[u].x), "+v"(raw[u].y), "+v"(raw[u].z), "+v"(raw[u].w));
#pragma unroll
                    for (int u = 0; u < kInFlight; ++u) widen8<DT>(raw[u], v[u]);
                } else {
#pragma unroll
                    for (int u = 0; u < kInFlight; ++u) load_vec<VEC>(xc + int64_t(id[u]) * ldx, v[u]);
#pragma unroll
                    for (int u = 0; u < kInFlight; ++u)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) asm volatile("" : "+v"(v[u][e]));
                }
#pragma unroll
                for (int u = 0; u < kInFlight; ++u)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[e] = (j0 + u < m_l) ? fmaf(wt[u], v[u][e], acc[e]) : acc[e];
            }
            if (op == TFGX_MEAN) {
                const float div = float(max(m_l, 1));
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] = acc[e] / div;
            }
            if (live && ok_l && c < ncols) {
                float* oc = out + (base + l) * ldo + col0 + int64_t(c) * VEC;
                if constexpr (kHalf) {
                    store8_f32(oc, out_vec, min(VEC, f_end - (col0 + c * VEC)), acc);      // the last chunk: masked per column
                } else if (VEC == 1 || out_vec) {
                    store_vec<VEC>(oc, acc);
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) oc[e] = acc[e];
                }
            }
        }
    }
}

__device__ __forceinline__ int lanes_for(int ncols)      // log2 of the smallest power of two >= ncols, at most 6
{
    int lg = 0;
    while (lg < 6 && (1 << lg) < ncols) ++lg;
    return lg;
}

// DT = TFGX_DT_F32, VEC = 4: x's rows start on 16 bytes and F >= 4 — float4 loads for the first F / 4 * 4 columns, scalar ones for
// the rest; VEC = 1: scalar loads throughout.  DT = TFGX_DT_BF16 / TFGX_DT_F16 (include/tfgx_minibatch_h16.h), VEC = 8: ceil(F / 8)
// 16-byte chunks cover the row, pad columns included, and there is no scalar pass.
// seed_dev != NULL (tfgx_nbrstatic_input_hop_f32): the seed is hop `hop`'s mix of the DEVICE word, and a negative row id is a
// dead slot — a row of zeros, count 0, no flag — not a refusal.
template <int DT, int VEC>
__global__ __launch_bounds__(kBlock) void samplereduce_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                             const float* __restrict__ w, int32_t n_nodes,
                                                             const int32_t* __restrict__ rows, int64_t n_rows, int tile_rows,
                                                             int k, int replace_when_short, uint64_t seed,
                                                             const uint64_t* __restrict__ seed_dev, int hop,
                                                             const typename ElemOf<DT>::type* __restrict__ x, int64_t ldx, int F,
                                                             int op, float* __restrict__ out, int64_t ldo, int out_vec,
                                                             int32_t* __restrict__ out_count, int32_t* __restrict__ bad_flag)
{
    __shared__ int32_t s_col_all[kWaves][kSlots];
    __shared__ float s_w_all[kWaves][kSlots];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    int32_t* s_col = s_col_all[wave];
    float* s_w = s_w_all[wave];
    if (seed_dev != nullptr) seed = hop_seed_from(seed_dev, hop);
    const int64_t n_tiles = (n_rows + tile_rows - 1) / tile_rows;
    const int64_t n_waves = int64_t(gridDim.x) * kWaves;
    for (int64_t tile = int64_t(blockIdx.x) * kWaves + wave; tile < n_tiles; tile += n_waves) {
        const int64_t base = tile * tile_rows;
        const int n_tile = int(min(int64_t(tile_rows), n_rows - base));
        // ---- phase 1: lane l draws row l of the tile into slots [l * k, l * k + m)
        int32_t r = 0;
        int s = 0, d = 0, m = 0, ok = 0;
        if (lane < n_tile) {
            r = rows[base + lane];
            if (r < 0 && seed_dev != nullptr) {
                ok = 1;                                                  // a dead slot: zeros (m stays 0)
                if (out_count != nullptr) out_count[base + lane] = 0;
            } else if (r < 0 || r >= n_nodes) {
                atomicOr(bad_flag, TFGX_SAMPLEREDUCE_BAD_RANGE);
            } else {
                ok = 1;
                s = row_ptr[r];
                d = row_ptr[r + 1] - s;
                m = sample_row_draws(d, k, replace_when_short);
                if (out_count != nullptr) out_count[base + lane] = m;
            }
        }
        if (lane < n_tile && m == 0 && k > 0) s_col[lane * k] = 0;      // what the reduce phase's clamped reads find: a valid id
        const bool is_long = m > 0 && sample_row_is_long(d, m);
        if (m > 0 && !is_long) sample_row_lane(col, w, uint64_t(r), s, d, lane * k, m, replace_when_short, seed, s_col, s_w);
        for (unsigned long long todo = __ballot(is_long); todo != 0; todo &= todo - 1) {
            const int l = __ffsll(todo) - 1;
            sample_row_wave(col, w, uint64_t(__shfl(r, l)), __shfl(s, l), __shfl(d, l), l * k, __shfl(m, l), replace_when_short,
                            seed, s_col, s_w, lane);
        }
        wave_sync();
        // ---- phase 2: reduce the drawn rows of x
        if constexpr (DT != TFGX_DT_F32) {
            const int nc = (F + kVec - 1) / kVec;
            reduce_tile<DT, kVec>(s_col, s_w, k, n_tile, base, m, ok, x, ldx, 0, nc, F, lanes_for(nc), op, out, ldo, out_vec != 0, lane);
        } else if constexpr (VEC == 4) {
            const int nv = F / 4, tail = F - nv * 4;
            reduce_tile<DT, 4>(s_col, s_w, k, n_tile, base, m, ok, x, ldx, 0, nv, F, lanes_for(nv), op, out, ldo, out_vec != 0, lane);
            if (tail > 0) reduce_tile<DT, 1>(s_col, s_w, k, n_tile, base, m, ok, x, ldx, nv * 4, tail, F, 2, op, out, ldo, false, lane);
        } else {
            reduce_tile<DT, 1>(s_col, s_w, k, n_tile, base, m, ok, x, ldx, 0, F, F, lanes_for(F), op, out, ldo, false, lane);
        }
        wave_sync();           // the next tile's draws overwrite these slots
    }
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_samplereduce_version(void) { return TFGX_SAMPLEREDUCE_ABI_VERSION; }

// every entry point, float32 and 16-bit: `fn` names the caller in every refusal; seed_dev NULL = the by-value seed; x_dtype
// TFGX_DT_F32 = a float table, else the 16-bit table of include/tfgx_minibatch_h16.h
static int samplereduce_launch(const char* fn, const int32_t* row_ptr, const int32_t* col, const float* w, int64_t n_nodes,
                               const int32_t* rows, int64_t n_rows, int32_t k, int32_t replace_when_short, uint64_t seed,
                               const uint64_t* seed_dev, int32_t hop, const void* x, int64_t ldx, int64_t F, int32_t x_dtype,
                               int32_t op, float* out, int64_t ldo, int32_t* out_count, int32_t* bad_flag, tfgx_stream_t stream)
{
    const bool half = x_dtype != TFGX_DT_F32;
    if (half && !is_h16(x_dtype)) return bad_arg(fn, "x_dtype must be TFGX_DT_BF16 or TFGX_DT_F16", x_dtype);
    if (int rc = check_size(fn, "n_nodes", n_nodes)) return rc;
    if (int rc = check_size(fn, "n_rows", n_rows)) return rc;
    if (k < 0) return bad_arg(fn, "k must not be negative", k);
    if (k > TFGX_SAMPLEREDUCE_MAX_DRAWS) return bad_arg(fn, "k is above TFGX_SAMPLEREDUCE_MAX_DRAWS = " TFGX_STR(TFGX_SAMPLEREDUCE_MAX_DRAWS), k);
    if (F < 1) return bad_arg(fn, "F must be at least 1", (long long)F);
    if (int rc = check_size(fn, "F", F)) return rc;
    if (ldx < F) return bad_arg(fn, "ldx must be at least F", (long long)ldx);
    if (half && ldx % kVec != 0) return bad_arg(fn, "ldx must be a multiple of 8: rows of a 16-bit table are 16-byte aligned", (long long)ldx);
    if (half && !aligned_to(x, 16)) return bad_arg(fn, "x must be 16-byte aligned: its address modulo 16", (long long)(reinterpret_cast<uintptr_t>(x) % 16));
    if (ldo < F) return bad_arg(fn, "ldo must be at least F", (long long)ldo);
    if (op != TFGX_SUM && op != TFGX_MEAN) return bad_arg(fn, "op must be TFGX_SUM or TFGX_MEAN", op);
    if (n_rows == 0) return TFGX_OK;
    if (rows == nullptr) return null_arg(fn, "rows");
    if (out == nullptr) return null_arg(fn, "out");
    if (bad_flag == nullptr) return null_arg(fn, "bad_flag");
    if (n_nodes > 0 && row_ptr == nullptr) return null_arg(fn, "row_ptr");
    if (n_nodes > 0 && col == nullptr) return null_arg(fn, "col");
    if (n_nodes > 0 && x == nullptr) return null_arg(fn, "x");

    const bool x_vec = !half && F >= 4 && ldx % 4 == 0 && aligned_to(x, 16);
    const bool out_vec = ldo % 4 == 0 && aligned_to(out, 16);
    // rows per tile: all a wave's slots hold, but no more than leaves the device a few thousand waves, and no fewer than the
    // reduce phase works on at once (64 / G rows)
    const int64_t cols_per_row = half ? (F + kVec - 1) / kVec : x_vec ? F / 4 : F;
    int at_once = 64;
    while (at_once > 1 && 64 / at_once < cols_per_row) at_once /= 2;
    int64_t tile_rows = (n_rows + 4095) / 4096;
    if (tile_rows < at_once) tile_rows = at_once;
    const int64_t fit = kSlots / (k > 0 ? k : 1);
    if (tile_rows > fit) tile_rows = fit;
    if (tile_rows > kWave) tile_rows = kWave;
    const int64_t n_tiles = (n_rows + tile_rows - 1) / tile_rows;
    const int grid = grid_for(n_tiles, kWaves);
#define TFGX_SAMPLEREDUCE_LAUNCH(DT, VEC, OUT_VEC)                                                                                   \
    samplereduce_kernel<DT, VEC><<<grid, kBlock, 0, as_stream(stream)>>>(                                                            \
        row_ptr, col, w, int32_t(n_nodes), rows, n_rows, int(tile_rows), k, replace_when_short, seed, seed_dev, hop,                 \
        static_cast<const ElemOf<DT>::type*>(x), ldx, int(F), op, out, ldo, OUT_VEC, out_count, bad_flag)
    if (x_dtype == TFGX_DT_BF16) TFGX_SAMPLEREDUCE_LAUNCH(TFGX_DT_BF16, kVec, out_vec ? 1 : 0);
    else if (x_dtype == TFGX_DT_F16) TFGX_SAMPLEREDUCE_LAUNCH(TFGX_DT_F16, kVec, out_vec ? 1 : 0);
    else if (x_vec) TFGX_SAMPLEREDUCE_LAUNCH(TFGX_DT_F32, 4, out_vec ? 1 : 0);
    else TFGX_SAMPLEREDUCE_LAUNCH(TFGX_DT_F32, 1, 0);
#undef TFGX_SAMPLEREDUCE_LAUNCH
    TFGX_LAUNCH_CHECK("samplereduce_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_samplereduce_f32(const int32_t* row_ptr, const int32_t* col, const float* w, int64_t n_nodes,
                                     const int32_t* rows, int64_t n_rows, int32_t k, int32_t replace_when_short, uint64_t seed,
                                     const float* x, int64_t ldx, int64_t F, int32_t op, float* out, int64_t ldo,
                                     int32_t* out_count, int32_t* bad_flag, tfgx_stream_t stream)
{
    TFGX_RANGE();
    return samplereduce_launch(__func__, row_ptr, col, w, n_nodes, rows, n_rows, k, replace_when_short, seed, nullptr, 0, x, ldx,
                               F, TFGX_DT_F32, op, out, ldo, out_count, bad_flag, stream);
}

// the seed-pointer forms: what they refuse before the shared launch
static int static_hop_args(const char* fn, const int32_t* node, int64_t n_rows, const uint64_t* seed, int32_t hop)
{
    if (hop < 0) return bad_arg(fn, "hop must not be negative", hop);
    if (n_rows > 0 && node == nullptr) return null_arg(fn, "node");
    if (n_rows > 0 && seed == nullptr) return null_arg(fn, "seed");
    return TFGX_OK;
}

// include/tfgx_nbrstatic.h: the same launch with the seed read from the device and dead slots as rows of zeros
extern "C" int tfgx_nbrstatic_input_hop_f32(const int32_t* row_ptr, const int32_t* col, const float* w, int64_t n_nodes,
                                            const int32_t* node, int64_t n_rows, int32_t k, int32_t replace_when_short,
                                            const uint64_t* seed, int32_t hop, const float* x, int64_t ldx, int64_t F, int32_t op,
                                            float* out, int64_t ldo, int32_t* out_count, int32_t* bad_flag, tfgx_stream_t stream)
{
    TFGX_RANGE();
    if (int rc = static_hop_args(__func__, node, n_rows, seed, hop)) return rc;
    return samplereduce_launch(__func__, row_ptr, col, w, n_nodes, node, n_rows, k, replace_when_short, 0, seed, hop, x, ldx, F,
                               TFGX_DT_F32, op, out, ldo, out_count, bad_flag, stream);
}

// include/tfgx_minibatch_h16.h: both forms over a 16-bit table
extern "C" int tfgx_minibatch_h16_version(void) { return TFGX_MINIBATCH_H16_ABI_VERSION; }

// x_dtype TFGX_DT_F32 is the float32 entry points' own: here it is refused like any other value outside the two 16-bit types
static int32_t h16_only(int32_t x_dtype) { return x_dtype == TFGX_DT_F32 ? -1 : x_dtype; }

extern "C" int tfgx_sample_reduce_h16(const int32_t* row_ptr, const int32_t* col, const float* w, int64_t n_nodes,
                                      const int32_t* rows, int64_t n_rows, int32_t k, int32_t replace_when_short, uint64_t seed,
                                      const void* x, int64_t ldx, int64_t F, int32_t x_dtype, int32_t op, float* out, int64_t ldo,
                                      int32_t* out_count, int32_t* bad_flag, tfgx_stream_t stream)
{
    TFGX_RANGE();
    return samplereduce_launch(__func__, row_ptr, col, w, n_nodes, rows, n_rows, k, replace_when_short, seed, nullptr, 0, x, ldx,
                               F, h16_only(x_dtype), op, out, ldo, out_count, bad_flag, stream);
}

extern "C" int tfgx_nbr_static_input_hop_h16(const int32_t* row_ptr, const int32_t* col, const float* w, int64_t n_nodes,
                                             const int32_t* node, int64_t n_rows, int32_t k, int32_t replace_when_short,
                                             const uint64_t* seed, int32_t hop, const void* x, int64_t ldx, int64_t F,
                                             int32_t x_dtype, int32_t op, float* out, int64_t ldo, int32_t* out_count,
                                             int32_t* bad_flag, tfgx_stream_t stream)
{
    TFGX_RANGE();
    if (int rc = static_hop_args(__func__, node, n_rows, seed, hop)) return rc;
    return samplereduce_launch(__func__, row_ptr, col, w, n_nodes, node, n_rows, k, replace_when_short, 0, seed, hop, x, ldx, F,
                               h16_only(x_dtype), op, out, ldo, out_count, bad_flag, stream);
}
