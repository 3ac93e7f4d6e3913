/* pgcn_dense_wide.h -- C ABI of lib/libpgcn_gemm.so, continued: the dense products of a layer for widths above 128.
 * Beside include/pgcn_gemm.h, whose conventions hold: row-major fp32, leading dimensions in elements; 0 success; -2 refused, nothing
 * launched (shape, alignment, a stride of 2^25 or more, a work-space that is too small); -1 errors with
 * pgcn_dense_wide_last_error(); the entry points never allocate and never synchronise; n == 0 returns 0 and launches nothing.
 * Source: <package>/gemm/pgcn_dense_wide.hip; binding: <package>/PGCN.py (wide_linear_relu_fused, wide_grad_input_fused,
 * wide_weight_grad_masked_fused), selected by tuning.dense_wide.
 *
 * Shapes: 4 <= fin, fout <= 1024, both multiples of 4, max(fin, fout) > 128.  Shapes with both widths up to 128 belong to the
 * kernels of pgcn_gemm.h and are answered -2 here, so every shape has one owner.  Streamed operands (X; G, Gm) need 16-byte aligned
 * bases and leading dimensions that are multiples of 4; every leading dimension of a streamed operand or result is below 2^25;
 * W and dW may have any alignment.  Arithmetic: v_mfma_f32_32x32x16_bf16 on the exact three-plane bf16 split, six partial products
 * smallest first, fp32 accumulation; the bits of one row of Y / dX depend on that row and on W only (not on n, the row's position
 * or the grid); dW is deterministic (no atomics, partial matrices added in a fixed order).
 *
 * Why a header of its own: tests/test_zz_dense_fused.py pins the names declared in pgcn_gemm.h (as for pgcn_wgrad_masked.h); what is
 * declared here is held to the library's exports by tests/test_dense_wide_exports.py. */
#ifndef PGCN_DENSE_WIDE_H
#define PGCN_DENSE_WIDE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 1: the entry points below exist (a binding checks this before it resolves them; a library without it keeps the library route) */
int pgcn_dense_wide_abi_version(void);
const char *pgcn_dense_wide_last_error(void);

/* bytes of work-space for the B-operand image of a K x N product (chunks of 64 x 128, 48 KB each): the forward takes
 * (K, N) = (fin, fout), the input gradient (fout, fin).  The work-space is 16-byte aligned and written by every call. */
int64_t pgcn_wide_image_ws_bytes(int32_t K, int32_t N);

/* Y (n x fout, ldy) = relu ? max(X . W^T, 0) : X . W^T;  X: n x fin (ldx);  W: fout x fin (ldw).  mask (optional): the sign mask of
 * Y in the layout of pgcn_linear_relu_f32 (n x ceil(fout / 32) words; bits of columns >= fout are 0).
 * step != NULL: dropout as pgcn_dropout_linear_relu_f32 -- Y = keep ? max(X . W^T, 0) * scale : 0, mask = sign AND keep, keep hashed
 * from (seed, *step, layer, row id, column), row_ids (optional, int64, 8-byte aligned): the global id of every row; relu is implied.
 * step == NULL: no dropout; row_ids, seed, layer and thr are ignored. */
int pgcn_wide_linear_relu_f32(const float *X, int64_t ldx, int64_t n, int32_t fin, const float *W, int64_t ldw, int32_t fout, float *Y,
                              int64_t ldy, int32_t relu, uint32_t *mask, const int64_t *row_ids, uint64_t seed, const int64_t *step,
                              uint32_t layer, uint32_t thr, void *ws, int64_t ws_bytes, void *stream);

/* Gm = mask ? G * scale : +0 (a select: a NaN of G under a cleared bit gives +0; mask NULL: every bit set), dX (n x fin, lddx) = Gm . W.
 * Gm (optional, n x fout, ldgm) is written when not NULL and must not be G: the rows of G are read once per 128 columns of dX. */
int pgcn_wide_grad_input_f32(const float *G, int64_t ldg, const uint32_t *mask, float scale, float *Gm, int64_t ldgm, int64_t n,
                             int32_t fout, const float *W, int64_t ldw, int32_t fin, float *dX, int64_t lddx, void *ws, int64_t ws_bytes,
                             void *stream);

/* floats of work-space of the weight gradient for these sizes (partial matrices; at most 32 MB) */
int64_t pgcn_wide_weight_grad_ws_elems(int64_t n, int32_t fout, int32_t fin);

/* dW (fout x fin, lddw) = Gm^T . X with Gm = mask ? G * scale : +0 formed in registers (mask NULL: every bit set).  G: n x fout (ldg),
 * X: n x fin (ldx), 4-byte aligned; ws: 16-byte aligned.  n == 0 leaves dW untouched (nothing is launched). */
int pgcn_wide_weight_grad_f32(const float *G, int64_t ldg, const uint32_t *mask, float scale, const float *X, int64_t ldx, int64_t n,
                              int32_t fout, int32_t fin, float *dW, int64_t lddw, float *ws, int64_t ws_elems, void *stream);

#ifdef __cplusplus
}
#endif
#endif
