// The neighbour sampler (RandomNeighborSampler.sample, tf_geometric/utils/graph_utils.py:667-772): the generator, the per-row
// bodies, and the ONE kernel pair and launcher that run them for the whole-graph sampler (tfgx_misc.hip: row r of the graph ->
// out row r), the row-list sampler (tfgx_nbrblock.hip: node rows[i] -> out row i) and the fixed-shape hop (tfgx_nbrstatic.hip:
// the same, the seed read from the device).  A body is parameterised by the ROW ID that keys the generator and by the OUTPUT
// OFFSET of the row; given the same (seed, row id, d, m, replace_when_short) every caller writes the same bits.  The fused input
// hop (tfgx_samplereduce.hip) runs the bodies from its own kernel: its rows are lanes of a tile.
#pragma once
#include "tfgx_common.h"

namespace tfgx {

// counter-based generator: a 64-bit mix of (seed, row, draw) — reproducible, order-independent, no state
__device__ __forceinline__ uint32_t draw_u32(uint64_t seed, uint64_t row, uint32_t i)
{
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (row * 0x100000001B3ull + i + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<uint32_t>((z ^ (z >> 31)) >> 32);
}
__device__ __forceinline__ int draw_below(uint64_t seed, uint64_t row, uint32_t i, int n)   // uniform in [0, n)
{
    return static_cast<int>((uint64_t(draw_u32(seed, row, i)) * uint64_t(n)) >> 32);
}

// the sampling seed of hop `hop` (0 = next to the seeds) from a seed kept in DEVICE memory: utils.hop_seed's mixing,
// (seed + (hop + 1) * 0x9E3779B97F4A7C15) mod 2^63, done by the kernel that draws (a wave-uniform address: one scalar load) —
// a hipGraph replay reads the value the captured sequence left there, never one frozen into the graph
__device__ __forceinline__ uint64_t hop_seed_from(const uint64_t* __restrict__ seed_dev, int hop)
{
    return (*seed_dev + uint64_t(hop + 1) * 0x9E3779B97F4A7C15ull) & 0x7FFFFFFFFFFFFFFFull;
}

constexpr int kSampleLongRow = 64;      // rows with more neighbours / draws than this get a whole wave (coalesced walks)

constexpr int kFloydMax = 32;            // Floyd's O(m^2) duplicate check only for few draws; otherwise one O(d) selection pass

__device__ __forceinline__ bool sample_row_is_long(int d, int m)
{
    return (d > kSampleLongRow && m > kFloydMax) || m > kSampleLongRow;
}

// how many neighbours a row of d draws at fan-out k: none from an empty row, k with replacement, otherwise no more than it has
__device__ __forceinline__ int sample_row_draws(int d, int k, int replace_when_short)
{
    return d <= 0 ? 0 : (replace_when_short ? k : min(d, k));
}

// ONE LANE samples m > 0 of the d neighbours at CSR positions [s, s + d) of row `r` into out_col / out_w [o, o + m); the row
// is not long (sample_row_is_long(d, m) is false)
__device__ __forceinline__ void sample_row_lane(const int32_t* __restrict__ col, const float* __restrict__ w, uint64_t r,
                                                int s, int d, int o, int m, int replace_when_short, uint64_t seed,
                                                int32_t* __restrict__ out_col, float* __restrict__ out_w)
{
    if (m >= d && !(replace_when_short && m > d)) {          // keep every neighbour, in order (:742-744)
        for (int i = 0; i < d; ++i) {
            out_col[o + i] = col[s + i];
            if (out_w) out_w[o + i] = w ? w[s + i] : 1.0f;
        }
        return;
    }
    if (m > d) {                                             // padding: m draws WITH replacement (:749)
        for (int i = 0; i < m; ++i) {
            const int t = draw_below(seed, r, uint32_t(i), d);
            out_col[o + i] = col[s + t];
            if (out_w) out_w[o + i] = w ? w[s + t] : 1.0f;
        }
        return;
    }
    if (m > kFloydMax) {
        // m < d, more than a few draws (ratio sampling): Knuth's selection sampling (Algorithm S) — one pass over
        // the d neighbours, position j is taken with probability (m - taken) / (d - j): uniform without replacement,
        // no scratch, neighbour order kept
        int taken = 0;
        for (int j = 0; j < d && taken < m; ++j) {
            if (draw_below(seed, r, uint32_t(j), d - j) < m - taken) {
                out_col[o + taken] = col[s + j];
                if (out_w) out_w[o + taken] = w ? w[s + j] : 1.0f;
                ++taken;
            }
        }
        return;
    }
    // m < d: Floyd's algorithm — m distinct positions of [0, d) with uniform probability, no replacement
    int chosen[kFloydMax];
    int c = 0;
    for (int j = d - m; j < d; ++j) {
        int t = draw_below(seed, r, uint32_t(j - (d - m)), j + 1);
        bool dup = false;
        for (int q = 0; q < c; ++q) dup |= (chosen[q] == t);
        chosen[c++] = dup ? j : t;
    }
    for (int i = 0; i < m; ++i) {
        out_col[o + i] = col[s + chosen[i]];
        if (out_w) out_w[o + i] = w ? w[s + chosen[i]] : 1.0f;
    }
}

// ONE WAVE (all 64 lanes, `lane` = the caller's lane id) samples a LONG row (sample_row_is_long(d, m), m > 0).
// keep-all and with-replacement rows are copied / drawn lane-parallel.  m < d: the row's d positions are cut into 64
// contiguous strata; with ONE uniform integer U in [0, d) per row, stratum [b0, b1) receives (m*b1 + U)/d - (m*b0 + U)/d of
// the m samples (integer divisions: never more than it holds, exactly m in total, output offsets in closed form, expectation
// m * len / d) and draws them by selection sampling (Algorithm S).  Neighbour order is kept and EVERY neighbour is included
// with probability exactly m / d, as with the reference's np.random.choice; the joint draw is systematic across strata rather
// than a uniform m-subset (lower variance).
__device__ __forceinline__ void sample_row_wave(const int32_t* __restrict__ col, const float* __restrict__ w, uint64_t r,
                                                int s, int d, int o, int m, int replace_when_short, uint64_t seed,
                                                int32_t* __restrict__ out_col, float* __restrict__ out_w, int lane)
{
    constexpr int WV = 64;
    if (m >= d && !(replace_when_short && m > d)) {          // keep every neighbour, in order
        for (int i = lane; i < d; i += WV) {
            out_col[o + i] = col[s + i];
            if (out_w) out_w[o + i] = w ? w[s + i] : 1.0f;
        }
        return;
    }
    if (m > d) {                                             // padding: m draws WITH replacement (same draws as one lane)
        for (int i = lane; i < m; i += WV) {
            const int t = draw_below(seed, r, uint32_t(i), d);
            out_col[o + i] = col[s + t];
            if (out_w) out_w[o + i] = w ? w[s + t] : 1.0f;
        }
        return;
    }
    const int b0 = int(int64_t(d) * lane / WV), b1 = int(int64_t(d) * (lane + 1) / WV);        // stratum [b0, b1)
    const int64_t U = draw_below(seed, r, 0xFFFFFFFFu, d);                                     // the row's random offset
    const int o0 = int((int64_t(m) * b0 + U) / d), ml = int((int64_t(m) * b1 + U) / d) - o0;   // its samples
    int taken = 0;
    for (int j = b0; j < b1 && taken < ml; ++j) {
        if (draw_below(seed, r, uint32_t(j), b1 - j) < ml - taken) {
            out_col[o + o0 + taken] = col[s + j];
            if (out_w) out_w[o + o0 + taken] = w ? w[s + j] : 1.0f;
            ++taken;
        }
    }
}

// ---- which rows a launch samples: a compile-time ROW SOURCE.  node(i, r, report) gives the node r whose neighbours output row i
// draws — r indexes row_ptr and keys the generator — or false for a row to pass over; seed() is the launch's seed; kListed says
// that the rows are a caller's list of ids (sample_row_is_empty).
struct GraphRows {                       // row i is node i of the graph: nothing to look up, nothing to refuse
    static constexpr bool kListed = false;
    uint64_t seed_;
    __device__ __forceinline__ bool node(int64_t i, int64_t& r, bool) const
    {
        r = i;
        return true;
    }
    __device__ __forceinline__ uint64_t seed() const { return seed_; }
};

struct ListedRows {                      // node ids[i], refused against [0, n_nodes) before anything is indexed by it: the lane
    static constexpr bool kListed = true;        // kernel (report) ORs flag_bit into *flag, the wave kernel passes over silently
    const int32_t* ids;
    int32_t n_nodes;
    int32_t* flag;
    int32_t flag_bit;
    uint64_t seed_;
    __device__ __forceinline__ bool node(int64_t i, int64_t& r, bool report) const
    {
        r = ids[i];
        if (r >= 0 && r < n_nodes) return true;
        if (report) atomicOr(flag, flag_bit);
        return false;
    }
    __device__ __forceinline__ uint64_t seed() const { return seed_; }
};

struct ListedRowsDeviceSeed {            // node ids[i]; a dead row (and an id the sampler cannot have produced) is passed over
    static constexpr bool kListed = true;        // with no flag; the seed is hop `hop`'s mix of the device word
    const int32_t* ids;
    int32_t n_nodes;
    const uint64_t* seed_dev;
    int hop;
    __device__ __forceinline__ bool node(int64_t i, int64_t& r, bool) const
    {
        r = ids[i];
        return r >= 0 && r < n_nodes;
    }
    __device__ __forceinline__ uint64_t seed() const { return hop_seed_from(seed_dev, hop); }
};

// a row that draws nothing.  The whole graph's out_ptr follows its row_ptr: only m == 0 is met.  In a list, draws may have been
// asked of a node without neighbours (d <= 0): nothing to read
template <class Rows>
__device__ __forceinline__ bool sample_row_is_empty(int d, int m)
{
    return Rows::kListed ? (m <= 0 || d <= 0) : m == 0;
}

// one lane per row: out row i holds out_ptr[i + 1] - out_ptr[i] sampled CSR positions' (col, w)
template <class Rows>
__global__ void sample_lane_per_row_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                           const float* __restrict__ w, int64_t n_rows,
                                           const int32_t* __restrict__ out_ptr, int replace_when_short, Rows rows,
                                           int32_t* __restrict__ out_col, float* __restrict__ out_w)
{
    const uint64_t seed = rows.seed();
    int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; i < n_rows; i += stride) {
        int64_t r;
        if (!rows.node(i, r, true)) continue;
        const int s = row_ptr[r], d = row_ptr[r + 1] - s;
        const int o = out_ptr[i], m = out_ptr[i + 1] - o;
        if (sample_row_is_empty<Rows>(d, m)) continue;
        if (sample_row_is_long(d, m)) continue;                   // sample_wave_per_row_kernel, a wave each
        sample_row_lane(col, w, uint64_t(r), s, d, o, m, replace_when_short, seed, out_col, out_w);
    }
}

// Rows with more than 64 neighbours or draws (all of a power-law graph's mass; hubs of 10^4 .. 10^5 neighbours): one WAVE
// per row instead of one lane — coalesced walks, no divergence between a hub and its wave-mates (R-MAT, ratio = 0.5:
// 43 ms -> see profiles/r02_skew_cliff_scan.jsonl).  The stratified draw is sample_row_wave.
template <class Rows>
__global__ __launch_bounds__(kBlock) void sample_wave_per_row_kernel(const int32_t* __restrict__ row_ptr,
                                                                     const int32_t* __restrict__ col,
                                                                     const float* __restrict__ w, int64_t n_rows,
                                                                     const int32_t* __restrict__ out_ptr,
                                                                     int replace_when_short, Rows rows,
                                                                     int32_t* __restrict__ out_col, float* __restrict__ out_w)
{
    constexpr int WV = 64;
    const uint64_t seed = rows.seed();
    const int lane = threadIdx.x % WV;
    int64_t i = (blockIdx.x * int64_t(kBlock) + threadIdx.x) / WV;
    const int64_t stride = int64_t(gridDim.x) * kBlock / WV;
    for (; i < n_rows; i += stride) {
        int64_t r;
        if (!rows.node(i, r, false)) continue;
        const int s = row_ptr[r], d = row_ptr[r + 1] - s;
        const int o = out_ptr[i], m = out_ptr[i + 1] - o;
        if (sample_row_is_empty<Rows>(d, m) || !sample_row_is_long(d, m)) continue;
        sample_row_wave(col, w, uint64_t(r), s, d, o, m, replace_when_short, seed, out_col, out_w, lane);
    }
}

// both launches of a sample on `stream`: a lane per row, then a wave for each row the lanes left (hubs) — a pass over the ids
// and out_ptr when there are none.  The second grid is capped at an ODD size: with a power-of-two row stride the hubs of an R-MAT
// graph — ids k * 2^16 — would all land in one wave slot.
template <class Rows>
inline int launch_sample_rows(const int32_t* row_ptr, const int32_t* col, const float* w, const Rows& rows, int64_t n_rows,
                              const int32_t* out_ptr, int replace_when_short, int32_t* out_col, float* out_w, hipStream_t stream)
{
    sample_lane_per_row_kernel<<<grid_for(n_rows, kBlock), kBlock, 0, stream>>>(row_ptr, col, w, n_rows, out_ptr,
                                                                                 replace_when_short, rows, out_col, out_w);
    TFGX_LAUNCH_CHECK("sample_lane_per_row_kernel");
    sample_wave_per_row_kernel<<<grid_for(n_rows * 64, kBlock, (1 << 14) - 3), kBlock, 0, stream>>>(
        row_ptr, col, w, n_rows, out_ptr, replace_when_short, rows, out_col, out_w);
    TFGX_LAUNCH_CHECK("sample_wave_per_row_kernel");
    return TFGX_OK;
}

}  // namespace tfgx
