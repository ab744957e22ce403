// A 16-byte vector of a 16-bit feature table (include/tfgx_h16.h) in registers: the widening every kernel that reads such a table
// shares, and the float32 store of the 8 columns it stands for.  Widening is exact for both types (bf16: a 16-bit shift, fp16:
// v_cvt_f32_f16), which is what lets a kernel over a 16-bit table return the float32 kernel's bits for the widened table.
#pragma once
#include "tfgx_common.h"
#include "../../include/tfgx_h16.h"

namespace tfgx {

constexpr int kVec = 8;      // elements per 16-byte vector of a 16-bit table

template <int DT>
__device__ __forceinline__ float widen1(uint32_t bits16)
{
    if constexpr (DT == TFGX_DT_BF16) return __uint_as_float(bits16 << 16);
    else return float(__builtin_bit_cast(_Float16, static_cast<unsigned short>(bits16)));
}

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
            v[2 * i] = widen1<DT>(u[i] & 0xFFFFu);
            v[2 * i + 1] = widen1<DT>(u[i] >> 16);
        }
    }
}

// 8 consecutive floats of a row, the first `nv` of them inside it: 16-byte stores for the whole halves when `vec` (the row and
// the chunk start on 16 bytes), one store per column otherwise.  Columns past nv are never written.
__device__ __forceinline__ void store8_f32(float* p, bool vec, int nv, const float (&v)[kVec])
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (vec && nv >= 4 * h + 4) {
            *reinterpret_cast<float4*>(p + 4 * h) = make_float4(v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * h + i < nv) p[4 * h + i] = v[4 * h + i];
        }
    }
}

inline bool is_h16(int32_t dt) { return dt == TFGX_DT_BF16 || dt == TFGX_DT_F16; }

}  // namespace tfgx
