// C = act(A[M,K] @ B[K,N] + bias) and dW = X^T @ G on the matrix cores: the float32 entry points of include/tfgx.h.
// The kernels, their launchers and the dispatcher live in tfgx_gemm_kernels.h as templates over the element type of A; this
// file instantiates them for float.  (tfgx_gemm_h16.hip instantiates them for the 16-bit tables of tfgx_gemm_h16.h.)
#include "tfgx_gemm_kernels.h"

using namespace tfgx;

#if TFGX_ROWS_EXPERIMENT == 3
// developer build only: read and clear the row kernel's in-kernel clocks (see gemm_rows_kernel)
extern "C" int tfgx_debug_rows_stats(uint64_t* out4)
{
    uint64_t z[16] = {0, 0, 0, 0, 0, ~0ull, 0, 0, ~0ull, 0, ~0ull, 0, 0, 0, 0, 0};
    TFGX_HIP_CHECK(hipDeviceSynchronize());
    TFGX_HIP_CHECK(hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_rows_dbg), sizeof(z)));
    TFGX_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_rows_dbg), z, sizeof(z)));
    return TFGX_OK;
}
#endif

#if TFGX_ROWS_EXPERIMENT == 3
extern "C" int tfgx_debug_rows_waves(uint64_t* out, int n_waves)
{
    TFGX_HIP_CHECK(hipDeviceSynchronize());
    TFGX_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rows_wave), sizeof(uint64_t) * 4 * size_t(n_waves)));
    return TFGX_OK;
}
#endif

extern "C" size_t tfgx_gemm_workspace_bytes(int64_t M, int64_t K, int64_t N)
{
    if (M <= 0 || K <= 0 || N <= 0) return 0;
    const int s = splitk_factor(generic_tiles(M, N), K);
    if (s > 1) return sizeof(float) * size_t(s) * size_t(M) * size_t(N);
    // the row kernel's tile counters (alignment slack included); whether the row kernel runs also depends on the pointers,
    // so this is an upper bound for shapes it can take
    const bool rows_shape = N <= 512 && K >= 32 && K % 4 == 0 && M >= 128 * 256;
    return (rows_shape && rows_dynamic_wanted(M)) ? kRowsCounterBytes + 128 : 0;
}

extern "C" int tfgx_gemm_bias_act_cols_f32(const float* A, int64_t lda, const float* B, int64_t ldb,
                                           const float* bias, int32_t act, int64_t act_cols, float* C, int64_t ldc,
                                           int64_t M, int64_t K, int64_t N, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    return tfgx_gemm_bias_act_cols_ws_f32(A, lda, B, ldb, bias, act, act_cols, C, ldc, M, K, N, nullptr, 0, stream_);
}

extern "C" int tfgx_gemm_bias_act_cols_ws_f32(const float* A, int64_t lda, const float* B, int64_t ldb,
                                              const float* bias, int32_t act, int64_t act_cols, float* C, int64_t ldc,
                                              int64_t M, int64_t K, int64_t N, void* workspace, size_t workspace_bytes,
                                              tfgx_stream_t stream_)
{
    return gemm_bias_act_cols_ws<float>(__func__, A, lda, B, ldb, bias, act, act_cols, C, ldc, M, K, N, workspace, workspace_bytes,
                                        stream_);
}

extern "C" int tfgx_gemm_describe(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, int32_t act,
                                  int64_t act_cols, const float* C, int64_t ldc, int64_t M, int64_t K, int64_t N,
                                  void* workspace, size_t workspace_bytes, char* buf, size_t buf_bytes)
{
    (void)bias;
    return gemm_describe<float>(__func__, A, lda, B, ldb, act, act_cols, C, ldc, M, K, N, workspace, workspace_bytes, buf, buf_bytes);
}

extern "C" int tfgx_gemm_bias_act_f32(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias,
                                      int32_t act, float* C, int64_t ldc, int64_t M, int64_t K, int64_t N,
                                      tfgx_stream_t stream)
{
    TFGX_RANGE();
    return tfgx_gemm_bias_act_cols_f32(A, lda, B, ldb, bias, act, N, C, ldc, M, K, N, stream);
}

extern "C" size_t tfgx_gemm_tn_workspace_bytes(int64_t M, int64_t Ka, int64_t N, int32_t want_bias)
{
    if (M <= 0 || Ka <= 0 || N <= 0) return 0;
    if (tn_use_direct()) {
        // (gated calls never split: they get the larger of the two figures)
        const TnDirectCfg d = tn_direct_config(M, Ka, N, want_bias != 0);
        size_t bytes = sizeof(float) * size_t(Ka + (want_bias ? 1 : 0)) * size_t(N) * size_t(d.wgs);
        if (tn_bias_by_column_sum(M, Ka, N, want_bias != 0, false)) {
            const TnDirectCfg d0 = tn_direct_config(M, Ka, N, false);
            const size_t split = (sizeof(float) * size_t(Ka) * size_t(N) * size_t(d0.wgs) + 255) / 256 * 256 +
                                 tfgx_column_sum_workspace_bytes(M, N);
            bytes = split > bytes ? split : bytes;
        }
        return bytes;
    }
    if (Ka > 2016) return 0;
    const TnCfg c = tn_config(M, Ka, N, want_bias != 0);
    return sizeof(float) * c.part_floats * size_t(c.wgs);
}

extern "C" int tfgx_gemm_tn_f32(const float* X, int64_t ldx, const float* G, int64_t ldg, int64_t M, int64_t Ka,
                                int64_t N, float* dW, int64_t ldw, float* db, void* workspace, size_t workspace_bytes,
                                tfgx_stream_t stream_)
{
    return tfgx_gemm_tn_gated_f32(X, ldx, G, ldg, nullptr, 0, M, Ka, N, dW, ldw, db, workspace, workspace_bytes, stream_);
}

extern "C" int tfgx_gemm_tn_gated_f32(const float* X, int64_t ldx, const float* G, int64_t ldg, const float* gate,
                                      int64_t ld_gate, int64_t M, int64_t Ka, int64_t N, float* dW, int64_t ldw, float* db,
                                      void* workspace, size_t workspace_bytes, tfgx_stream_t stream_)
{
    return gemm_tn_gated<float>(__func__, X, ldx, G, ldg, gate, ld_gate, M, Ka, N, dW, ldw, db, workspace, workspace_bytes, stream_);
}

// out[c, r] = in[r, c]  (the [K, N] kernel of a dense layer, transposed for d/dx = g @ kernel^T on the forward GEMM)
namespace tfgx {
namespace {
__global__ void transpose_kernel(const float* __restrict__ in, int64_t ldi, int64_t rows, int64_t cols,
                                 float* __restrict__ out, int64_t ldo)
{
    __shared__ float tile[32][33];
    const int64_t r0 = int64_t(blockIdx.y) * 32, c0 = int64_t(blockIdx.x) * 32;
    for (int dy = threadIdx.y; dy < 32; dy += blockDim.y) {
        const int64_t r = r0 + dy, c = c0 + threadIdx.x;
        tile[dy][threadIdx.x] = (r < rows && c < cols) ? in[r * ldi + c] : 0.0f;
    }
    __syncthreads();
    for (int dy = threadIdx.y; dy < 32; dy += blockDim.y) {
        const int64_t c = c0 + dy, r = r0 + threadIdx.x;
        if (c < cols && r < rows) out[c * ldo + r] = tile[threadIdx.x][dy];
    }
}
}  // namespace
}  // namespace tfgx

extern "C" int tfgx_transpose_f32(const float* in, int64_t ldi, int64_t rows, int64_t cols, float* out, int64_t ldo,
                                  tfgx_stream_t stream)
{
    TFGX_RANGE();
    TFGX_REQUIRE(rows >= 0 && cols >= 0 && ldi >= cols && ldo >= rows, "bad shape");
    if (rows == 0 || cols == 0) return TFGX_OK;
    TFGX_REQUIRE(in && out, "null pointer");
    dim3 grid(unsigned((cols + 31) / 32), unsigned((rows + 31) / 32), 1), block(32, 8, 1);
    tfgx::transpose_kernel<<<grid, block, 0, as_stream(stream)>>>(in, ldi, rows, cols, out, ldo);
    TFGX_LAUNCH_CHECK("transpose_kernel");
    return TFGX_OK;
}
