// What the two fused aggregate -> project launches share (tfgx_fused.hip: float32 table, tfgx_fused_h16.hip: bf16 / fp16
// table): the LDS geometry and its budget, the projection half of the kernel arguments, the LDS set-up, the CONSUMER — the
// hand-over of a finished tile, the MFMA loops, the epilogue and the stores — and the host side of a launch.  The producers
// (how a wave reduces its destination row) are the kernels' own.  Internal: no part of the C ABI.
#pragma once
#include "tfgx_common.h"
#include "tfgx_mfma.h"

namespace tfgx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTileRows = 64;
constexpr int kLda = kTileRows + 1;
constexpr int kBufs = 2;
constexpr int kFusedThreads = 1024;
// 32-column blocks per consumer job, so up to eight jobs per tile.  2 measured best: 4 halves the jobs, 1 loses the shared A
// operand.  On tiles of short rows (the tail of a power-law graph in walk order) the producers are done in less than one wave's
// multiplication time, and a single consumer wave was what the launch waited for
constexpr int kJB = 2;
constexpr size_t kFusedLdsLimit = 160 * 1024;
constexpr int kFusedMaxDev = 64;

inline size_t fused_lds_bytes(int kp, int ldw)
{
    return sizeof(float) * (size_t(kp) * ldw + size_t(kBufs) * kp * kLda) + sizeof(int) * (16 + kBufs * kTileRows);
}

// Columns of B kept in LDS for a [kp, np] projection (np = N rounded up to 128): all of them when B and the two tiles fit,
// else the largest multiple of 64 (one consumer job = 64 columns) that does; 0 = not even 64 columns fit.
inline int fused_resident_cols(int kp, int np)
{
    for (int nl = np; nl >= 64; nl -= 64)
        if (fused_lds_bytes(kp, nl + 8) <= kFusedLdsLimit) return nl;
    return 0;
}

// The projection and geometry half of the kernel arguments; FArgs / FHArgs add their producer's members.
struct FusedProj {
    const float* B;
    int64_t ldb;
    const float* bias;
    int32_t act;
    int32_t N;
    float* C;
    int64_t ldc;
    int32_t KP;        // F rounded up to even (the MFMA consumes two k per step)
    int32_t n_blocks;  // 32-column output blocks, rounded up to a multiple of 4
    int32_t LDW;       // NL + 8
    int32_t NL;        // columns of B resident in LDS (multiple of 64); columns >= NL: B operand from global
    int64_t n_tiles;
    int64_t n_dst;
    int32_t F;         // columns of the aggregate = rows of B
    // skewed plans: slot i of the launch reduces destination row row_order[i] (the plan's rows sorted by length), so the 64
    // rows of a tile are of similar length and no lane group holds a tile back; NULL: i
    const int32_t* row_order;
};

inline void fused_fill_proj(FusedProj& a, const tfgx_reduce_args* p, const float* B, int64_t ldb, const float* bias, int32_t act,
                            float* C, int64_t ldc, int64_t N)
{
    a.B = B; a.ldb = ldb; a.bias = bias; a.act = act; a.N = int32_t(N); a.C = C; a.ldc = ldc;
    a.KP = int32_t((p->F + 1) / 2 * 2);
    a.n_blocks = int32_t((N + 127) / 128) * 4;          // 32-column blocks, in groups of four (columns >= N are zero in LDS)
    a.NL = fused_resident_cols(a.KP, 32 * a.n_blocks);
    a.LDW = a.NL + 8;
    a.n_tiles = (p->n_dst + kTileRows - 1) / kTileRows;
    a.n_dst = p->n_dst;
    a.F = int32_t(p->F);
    a.row_order = p->row_order;
}

// Power-law plans, before the fused launch: every chunk of a hub row is reduced like an ordinary row into hub_scratch (the
// unfused path's step 2) by the caller's own tfgx_segment_reduce_*; these are that launch's arguments.
inline tfgx_reduce_args fused_hub_chunk_args(const tfgx_reduce_args* p)
{
    tfgx_reduce_args c = *p;
    c.row_begin = p->hub_chunk_begin; c.row_end = p->hub_chunk_end; c.rp_stride = 1;
    c.n_dst = p->n_hub_chunks; c.out = p->hub_scratch; c.ldo = p->F;
    c.op = TFGX_SUM; c.act = TFGX_ACT_NONE; c.accumulate = 0;
    c.self_coef = nullptr; c.bias = nullptr; c.add_x = nullptr; c.mean_count = nullptr;
    c.hub_threshold = 0; c.hub_rows = nullptr; c.hub_chunk_ptr = nullptr; c.hub_chunk_begin = nullptr;
    c.hub_chunk_end = nullptr; c.n_hub_rows = 0; c.n_hub_chunks = 0; c.hub_scratch = nullptr;
    c.row_order = nullptr;          // (a walk order names DESTINATION rows; the chunk launch walks chunks)
    c.hub_order_slot = nullptr;
    return c;
}

// The current device and its compute-unit count, kept per DEVICE (one process may drive several).  fn: the entry point a
// refusal names.
inline int fused_device_cus(const char* fn, int* dev_out, int* cus_out)
{
    static int cus_of[kFusedMaxDev] = {0};
    int dev = 0;
    TFGX_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= kFusedMaxDev) {
        set_error("%s: %s", fn, "device ordinal out of range");
        return TFGX_ERR_INVALID_ARG;
    }
    if (cus_of[dev] == 0) {
        hipDeviceProp_t prop;
        TFGX_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
        cus_of[dev] = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    *dev_out = dev;
    *cus_out = cus_of[dev];
    return TFGX_OK;
}

// One persistent workgroup per CU (or per tile, if fewer); the dynamic-LDS attribute is set once per DEVICE and instantiation.
template <auto KERNEL, typename ARGS>
int fused_launch(const char* fn, const char* kernel_name, const ARGS& a, hipStream_t stream)
{
    static bool attr_set[kFusedMaxDev] = {false};
    int dev = 0, cus = 0;
    const int rc = fused_device_cus(fn, &dev, &cus);
    if (rc != TFGX_OK) return rc;
    if (!attr_set[dev]) {
        TFGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           int(kFusedLdsLimit)));
        attr_set[dev] = true;
    }
    const int64_t wgs = a.n_tiles < cus ? a.n_tiles : cus;
    KERNEL<<<dim3(unsigned(wgs)), dim3(kFusedThreads), fused_lds_bytes(a.KP, a.LDW), stream>>>(a);
    TFGX_LAUNCH_CHECK(kernel_name);
    return TFGX_OK;
}

template <int G>
__device__ __forceinline__ int bcast_i(int v, int j) { return __shfl(v, j, G); }
template <int G>
__device__ __forceinline__ float bcast_f(float v, int j) { return __shfl(v, j, G); }

struct FusedLds {
    float* Ws;      // [KP][LDW]
    float* At;      // [kBufs][KP][kLda]
    int* ctrl;      // [0] next unit | [1 + b] arrivals of buffer b | [1 + kBufs + b] done seq | [6 + b] finished jobs of buffer b's tile
    int* rowid;     // [kBufs][kTileRows]: the destination row of each tile slot (row_order)
};

// Carves the dynamic LDS up, loads the resident columns of B, zeroes the tiles and the counters; ends in the launch's only
// workgroup barrier.
__device__ __forceinline__ FusedLds fused_lds_init(const FusedProj& a, float* lds)
{
    FusedLds s;
    s.Ws = lds;
    s.At = s.Ws + a.KP * a.LDW;
    s.ctrl = reinterpret_cast<int*>(s.At + kBufs * a.KP * kLda);
    s.rowid = s.ctrl + 16;
    const int tid = threadIdx.x;
    for (int i = tid; i < a.KP * a.LDW; i += kFusedThreads) {
        const int k = i / a.LDW, n = i - k * a.LDW;
        s.Ws[i] = (k < a.F && n < a.N && n < a.NL) ? a.B[int64_t(k) * a.ldb + n] : 0.0f;
    }
    for (int i = tid; i < kBufs * a.KP * kLda; i += kFusedThreads) s.At[i] = 0.0f;      // rows k >= F stay zero for good
    if (tid < 16) s.ctrl[tid] = 0;
    __syncthreads();
    return s;
}

// Before a wave stores its row into buffer buf for tile q: wait until the buffer's previous tile (q - kBufs) has been multiplied.
__device__ __forceinline__ void fused_wait_buffer(const FusedLds& s, int q, int buf)
{
    if (q >= kBufs) {
        volatile int* done = s.ctrl + 1 + kBufs + buf;
        while (*done < q - kBufs + 1) __builtin_amdgcn_s_sleep(1);
        __threadfence_block();
    }
}

// The consumer.  Called by every wave once it has stored its unit (one of UNITS) of tile q, transposed, into buffer buf — and,
// in walk order, the unit's destination rows into rowid.  Counts the arrival; the last arrivers of the tile each multiply ONE
// 32-row x (32 kJB)-column block of it (the last one at once, the ones before it as soon as the tile is complete) ->
// C[tile rows, :] = act(At^T @ Ws + bias), while the earlier arrivers return to reduce the next tile into the other buffer.
// The last job to finish hands the buffer back.  No workgroup barrier: a buffer is re-used only after its `done` sequence
// number says the previous occupant has been multiplied (fused_wait_buffer).
template <int UNITS>
__device__ __forceinline__ void fused_arrive_and_multiply(const FusedProj& a, const FusedLds& s, int q, int buf, int64_t tile,
                                                          int lane64)
{
    constexpr int JB = kJB;
    int* const ctrl = s.ctrl;
    const float* ab = s.At + buf * a.KP * kLda;
    const int l31 = lane64 & 31, kh = lane64 >> 5;
    const bool vec_store = (a.N % 4 == 0) && (a.ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.C) & 15) == 0);      // wave-uniform
    __threadfence_block();
    int arrived = 0;
    if (lane64 == 0) arrived = atomicAdd(&ctrl[1 + buf], 1);
    arrived = __builtin_amdgcn_readfirstlane(arrived);
    const int njobs = 2 * (a.n_blocks / JB);             // 4 (N <= 128) or 8: never more than UNITS
    if (arrived < UNITS - njobs) return;

    const int job = UNITS - 1 - arrived;                 // the last arriver takes block 0, the one before it block 1, ...
    if (job > 0) {
        volatile int* arr = ctrl + 1 + buf;
        while (*arr < UNITS) __builtin_amdgcn_s_sleep(1);
    }
    __threadfence_block();
    const int mb = job & 1, nb0 = (job >> 1) * JB;       // n_blocks is a multiple of 4 (zero-padded columns of Ws)
    {
        f32x16 c4[JB];
#pragma unroll
        for (int jb = 0; jb < JB; ++jb)
#pragma unroll
            for (int t = 0; t < 16; ++t) c4[jb][t] = 0.0f;
        const float* ap = ab + kh * kLda + mb * 32 + l31;
        const int pairs = a.KP / 2;
        int pr = 0;
        if (nb0 * 32 < a.NL) {
            // B resident in LDS.  KU k-pairs per step: all (1 + JB) * KU LDS reads of a step are issued before its
            // JB * KU MFMAs (a read-wait-multiply chain per MFMA left the single consumer wave at ~2.5x the MFMA time
            // and the producers waiting for buffers)
            const float* bp = s.Ws + kh * a.LDW + nb0 * 32 + l31;
            constexpr int KU = 4;
            for (; pr + KU <= pairs; pr += KU) {
                float av[KU], bv[KU][JB];
#pragma unroll
                for (int t = 0; t < KU; ++t) {
                    av[t] = ap[(2 * (pr + t)) * kLda];
#pragma unroll
                    for (int jb = 0; jb < JB; ++jb) bv[t][jb] = bp[(2 * (pr + t)) * a.LDW + jb * 32];
                }
                __builtin_amdgcn_sched_barrier(0);      // left alone the scheduler sinks every read next to its MFMA
#pragma unroll
                for (int t = 0; t < KU; ++t)
#pragma unroll
                    for (int jb = 0; jb < JB; ++jb)
                        c4[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[t][jb], c4[jb], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            for (; pr < pairs; ++pr) {
                const float av = ap[(2 * pr) * kLda];
                float bv[JB];
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) bv[jb] = bp[(2 * pr) * a.LDW + jb * 32];
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) c4[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[jb], c4[jb], 0, 0, 0);
            }
        } else {
            // B columns past the resident ones: the operand comes from global memory (L2: every workgroup re-reads the
            // same <= 128 KB for every tile).  Lane (l31, kh) reads B[2 pr + kh][col]: two 128-byte row segments per
            // load; KG k-pairs = JB * KG loads in flight per wave before the first MFMA of the step.  Columns >= N read
            // column N - 1 (never stored).
            const float* gp[JB];
#pragma unroll
            for (int jb = 0; jb < JB; ++jb) {
                const int gn = (nb0 + jb) * 32 + l31;
                gp[jb] = a.B + int64_t(kh) * a.ldb + (gn < a.N ? gn : a.N - 1);
            }
            constexpr int KG = 8;
            for (; pr + KG <= pairs; pr += KG) {
                float av[KG], bv[KG][JB];
#pragma unroll
                for (int t = 0; t < KG; ++t)
#pragma unroll
                    for (int jb = 0; jb < JB; ++jb) bv[t][jb] = gp[jb][int64_t(2 * (pr + t)) * a.ldb];
#pragma unroll
                for (int t = 0; t < KG; ++t) av[t] = ap[(2 * (pr + t)) * kLda];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < KG; ++t)
#pragma unroll
                    for (int jb = 0; jb < JB; ++jb)
                        c4[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[t][jb], c4[jb], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            for (; pr < pairs; ++pr) {
                const float av = ap[(2 * pr) * kLda];
                float bv[JB];
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) bv[jb] = (2 * pr + kh < a.F) ? gp[jb][int64_t(2 * pr) * a.ldb] : 0.0f;
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) c4[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[jb], c4[jb], 0, 0, 0);
            }
        }
        // D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).  Two phases on purpose (as in
        // tfgx_gemm.hip): bias + activation IN PLACE first, then every store reads its own accumulator register —
        // results computed into a temporary right before each store make the compiler drain vmcnt(0) between
        // consecutive stores (measured here: 2.0 ms of the 10.8 ms launch went into 128 serialised stores per tile)
#pragma unroll
        for (int jb = 0; jb < JB; ++jb) {
            const int gn = (nb0 + jb) * 32 + l31;
            const float bv = (a.bias && gn < a.N) ? a.bias[gn] : 0.0f;
#pragma unroll
            for (int t = 0; t < 16; ++t) c4[jb][t] = apply_act(c4[jb][t] + bv, a.act);
        }
        const int64_t row0 = tile * kTileRows + mb * 32 + 4 * kh;
        const bool full = tile * kTileRows + kTileRows <= a.n_dst;
        if (a.row_order != nullptr && !vec_store) {     // walk order without 16-byte stores (odd N / unaligned C)
            // walk order: tile slot -> destination row through the ids the producers left in LDS
            const int* rid = s.rowid + buf * kTileRows + mb * 32 + 4 * kh;
#pragma unroll
            for (int jb = 0; jb < JB; ++jb) {
                const int gn = (nb0 + jb) * 32 + l31;
                if (gn >= a.N) continue;
#pragma unroll
                for (int t = 0; t < 16; ++t) {
                    const int rr = rid[(t & 3) + 8 * (t >> 2)];
                    if (rr >= 0) __builtin_nontemporal_store(c4[jb][t], a.C + int64_t(rr) * a.ldc + gn);
                }
            }
        } else if (vec_store && (full || a.row_order != nullptr)) {
            // 16-byte stores through a quad transpose of the accumulators (tfgx_mfma.h): 8 instead of 32 store
            // instructions per job; lane i of a quad ends with row 8 g + i + 4 kh, columns 4 q .. 4 q + 3
            const int qi = lane64 & 3, qc = (l31 >> 2) * 4;
            typedef float f32x4s __attribute__((ext_vector_type(4)));
            // destination rows of this lane's four register groups (g): natural order = ONE multiply + adds; walk
            // order = the ids the producers left in LDS (-1: past the end)
            int64_t roff[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int sl = mb * 32 + 8 * g + qi + 4 * kh;
                const int64_t rr = a.row_order != nullptr ? int64_t(s.rowid[buf * kTileRows + sl]) : tile * kTileRows + sl;
                roff[g] = rr >= 0 ? rr * a.ldc : int64_t(-1);
            }
#pragma unroll
            for (int jb = 0; jb < JB; ++jb) {
                float r4[4][4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {          // (every lane takes part in the quad permutes)
#pragma unroll
                    for (int k = 0; k < 4; ++k) r4[g][k] = c4[jb][4 * g + k];
                    quad_transpose4(r4[g], lane64);
                }
                const int gn = (nb0 + jb) * 32 + qc;
                if (gn < a.N) {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (roff[g] >= 0)
                            __builtin_nontemporal_store(f32x4s{r4[g][0], r4[g][1], r4[g][2], r4[g][3]},
                                                        reinterpret_cast<f32x4s*>(a.C + roff[g] + gn));
                }
            }
        } else {
#pragma unroll
            for (int jb = 0; jb < JB; ++jb) {
                const int gn = (nb0 + jb) * 32 + l31;
                if (gn >= a.N) continue;
                float* cp = a.C + row0 * a.ldc + gn;
                if (full) {
                    // streaming (non-temporal) stores: the output is written once and not read by this launch; kept out
                    // of the caches it does not evict source rows the gather still hits there
#pragma unroll
                    for (int t = 0; t < 16; ++t)
                        __builtin_nontemporal_store(c4[jb][t], cp + int64_t((t & 3) + 8 * (t >> 2)) * a.ldc);
                } else {
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        const int dr = (t & 3) + 8 * (t >> 2);
                        if (row0 + dr < a.n_dst) cp[int64_t(dr) * a.ldc] = c4[jb][t];
                    }
                }
            }
        }
    }
    __threadfence_block();
    int fin = 0;
    if (lane64 == 0) fin = atomicAdd(&ctrl[6 + buf], 1);
    fin = __builtin_amdgcn_readfirstlane(fin);
    if (fin == njobs - 1) {
        // the last job to finish hands the buffer back (wave-uniform branch; every lane stores the same values: no
        // single-lane branch around the hand-over)
        ctrl[1 + buf] = 0;
        ctrl[6 + buf] = 0;
        __threadfence_block();
        *reinterpret_cast<volatile int*>(ctrl + 1 + kBufs + buf) = q + 1;
    }
}

}  // namespace
}  // namespace tfgx
