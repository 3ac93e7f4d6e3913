/* pgcn_wgrad_masked.h -- C ABI of lib/libpgcn_gemm.so, continued: the weight gradient of a fused layer without Gm in memory.
 * Beside include/pgcn_gemm.h (whose conventions hold: row-major fp32, leading dimensions in elements, 0 / -2 refused, nothing
 * launched / -1 errors with pgcn_wgrad_last_error(); never allocates, never synchronises).  Source: <package>/gemm/pgcn_wgrad.hip;
 * binding: <package>/PGCN.py (weight_grad_masked_call).
 *
 * Why a header of its own and not two more declarations beside pgcn_linear_weight_grad_f32: tests/test_zz_dense_fused.py holds the
 * pgcn_(linear|dense|wgrad|sign)_* names declared in pgcn_gemm.h to an exact list, and that test is a fixed yardstick.  What is
 * declared here is held to the library's exports by tests/test_wgrad_masked_exports.py in the same way. */
#ifndef PGCN_WGRAD_MASKED_H
#define PGCN_WGRAD_MASKED_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 1: pgcn_linear_weight_grad_masked_f32 below exists (a binding checks this before it resolves it; an older library takes the
 * route through Gm) */
int pgcn_wgrad_masked_abi_version(void);

/* The same product on the Gm that the input gradient would have written, without that matrix: Gm[i][c] = bit c of the mask's row i ?
 * G[i][c] * scale : +0, formed in registers (a select: NaN / Inf of G under a cleared bit contribute +0) -- bit-identical to
 * pgcn_linear_weight_grad_f32 on Gm.  mask: n x ceil(fout / 32) words in the sign-mask layout of pgcn_linear_relu_f32, or NULL
 * (every bit set); scale: 1 for a plain ReLU layer, 1 / (1 - p) under dropout.  mask == NULL with scale == 1 is
 * pgcn_linear_weight_grad_f32 itself.  Operands, work-space and return codes as above. */
int pgcn_linear_weight_grad_masked_f32(const float *G, int64_t ldg, const int32_t *mask, float scale, const float *X, int64_t ldx,
                                       int64_t n, int32_t fout, int32_t fin, float *dW, int64_t lddw, float *ws, int64_t ws_elems,
                                       void *stream);

#ifdef __cplusplus
}
#endif
#endif
