// The dense GEMM and its weight gradient over a 16-BIT feature table (bf16 / fp16 storage, fp32 arithmetic):
// include/tfgx_gemm_h16.h.  The kernels, launchers and the dispatcher are the templates of tfgx_gemm_kernels.h — the ones
// tfgx_gemm.hip instantiates for float — instantiated here for bf16_t and f16_t; this file adds only the checks of the
// table's own layout.  A translation unit of its own: its instantiations compile beside the float32 ones.
#include "tfgx_gemm_kernels.h"
#include "../../include/tfgx_gemm_h16.h"

using namespace tfgx;

extern "C" int tfgx_gemm_h16_version(void) { return TFGX_GEMM_H16_ABI_VERSION; }

// the table's own layout (the float32 entry's checks follow in the shared template)
static int check_table(const char* who, const void* A, int32_t dtype, int64_t ld, int64_t K)
{
    TFGX_REQUIRE_AS(who, dtype == TFGX_DT_BF16 || dtype == TFGX_DT_F16, "dtype must be TFGX_DT_BF16 or TFGX_DT_F16");
    TFGX_REQUIRE_AS(who, ld % 8 == 0, "lda / ldx must be a multiple of 8 elements (16-byte aligned rows)");
    TFGX_REQUIRE_AS(who, aligned_to(A, 16), "A / X must be 16-byte aligned");
    TFGX_REQUIRE_AS(who, ld >= K, "lda / ldx smaller than K: leading dimension too small");
    TFGX_REQUIRE_AS(who, ld < (int64_t(1) << 25), "lda / ldx too large");      // the row kernel's 32-bit per-lane byte offsets
    return TFGX_OK;
}

extern "C" int tfgx_gemm_bias_act_cols_ws_h16(const void* A, int32_t a_dtype, int64_t lda, const float* B, int64_t ldb,
                                              const float* bias, int32_t act, int64_t act_cols, float* C, int64_t ldc, int64_t M,
                                              int64_t K, int64_t N, void* workspace, size_t workspace_bytes, tfgx_stream_t stream)
{
    const int rc = check_table(__func__, A, a_dtype, lda, K);
    if (rc != TFGX_OK) return rc;
    if (a_dtype == TFGX_DT_BF16)
        return gemm_bias_act_cols_ws<bf16_t>(__func__, static_cast<const bf16_t*>(A), lda, B, ldb, bias, act, act_cols, C, ldc, M, K, N,
                                             workspace, workspace_bytes, stream);
    return gemm_bias_act_cols_ws<f16_t>(__func__, static_cast<const f16_t*>(A), lda, B, ldb, bias, act, act_cols, C, ldc, M, K, N,
                                        workspace, workspace_bytes, stream);
}

extern "C" int tfgx_gemm_h16_describe(const void* A, int32_t a_dtype, int64_t lda, const float* B, int64_t ldb, const float* bias,
                                      int32_t act, int64_t act_cols, const float* C, int64_t ldc, int64_t M, int64_t K, int64_t N,
                                      void* workspace, size_t workspace_bytes, char* buf, size_t buf_bytes)
{
    (void)bias;
    TFGX_REQUIRE(buf != nullptr && buf_bytes > 0, "null argument");
    buf[0] = 0;
    const int rc = check_table(__func__, A, a_dtype, lda, K);
    if (rc != TFGX_OK) return rc;
    if (a_dtype == TFGX_DT_BF16)
        return gemm_describe<bf16_t>(__func__, static_cast<const bf16_t*>(A), lda, B, ldb, act, act_cols, C, ldc, M, K, N, workspace,
                                     workspace_bytes, buf, buf_bytes);
    return gemm_describe<f16_t>(__func__, static_cast<const f16_t*>(A), lda, B, ldb, act, act_cols, C, ldc, M, K, N, workspace,
                                workspace_bytes, buf, buf_bytes);
}

extern "C" int tfgx_gemm_tn_gated_h16(const void* X, int32_t x_dtype, int64_t ldx, const float* G, int64_t ldg, const float* gate,
                                      int64_t ld_gate, int64_t M, int64_t Ka, int64_t N, float* dW, int64_t ldw, float* db,
                                      void* workspace, size_t workspace_bytes, tfgx_stream_t stream)
{
    const int rc = check_table(__func__, X, x_dtype, ldx, Ka);
    if (rc != TFGX_OK) return rc;
    TFGX_REQUIRE(tn_use_direct(), "TFGX_TN_DIRECT=0: the LDS-staged kernel reads float32 only");
    if (x_dtype == TFGX_DT_BF16)
        return gemm_tn_gated<bf16_t>(__func__, static_cast<const bf16_t*>(X), ldx, G, ldg, gate, ld_gate, M, Ka, N, dW, ldw, db,
                                     workspace, workspace_bytes, stream);
    return gemm_tn_gated<f16_t>(__func__, static_cast<const f16_t*>(X), ldx, G, ldg, gate, ld_gate, M, Ka, N, dW, ldw, db, workspace,
                                workspace_bytes, stream);
}
