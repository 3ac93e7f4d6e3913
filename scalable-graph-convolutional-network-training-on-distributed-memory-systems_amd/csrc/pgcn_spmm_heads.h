// pgcn_spmm_heads.h -- what the attention gather kernels of pgcn_spmm_heads.hip (rows of up to 256 columns) and
// pgcn_spmm_heads_wide.hip (257 to 1024 columns) share: the kernel argument records and the cross-lane moves of the
// 16-lane reductions.  Everything has internal linkage: each translation unit compiles its own copy.
#ifndef PGCN_SPMM_HEADS_H
#define PGCN_SPMM_HEADS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgcn_internal.h"

namespace {

using f32x2 = __attribute__((ext_vector_type(2))) float;

// x of another lane of the same 16-lane row through the DPP network (CTRL: 0x120 + n = row_ror:n, 0x00-0xFF = quad_perm)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
// lane ^ 4 inside a 16-lane row: row_shl:4 serves the lanes of banks 0 and 2, row_shr:4 those of banks 1 and 3
__device__ __forceinline__ float dpp_xor4(float x) {
    const int v = __float_as_int(x);
    int r = __builtin_amdgcn_update_dpp(0, v, 0x104, 0xF, 0x5, false);
    r = __builtin_amdgcn_update_dpp(r, v, 0x114, 0xF, 0xA, false);
    return __int_as_float(r);
}

struct SliceSeg { int64_t v[PGCN_MAX_SLICES + 1]; };

struct Recompute {               // RECOMPUTE: alpha from (rowstat of the entry's column, s2 of the task's row)
    const float4 *rowstat;       // [ncols x KH] (s1, m, 1/D, exp(-m) or 0)
    const float *s2;             // [nrows x lds2]
    int64_t lds2;
    int64_t nrows;
    float slope;
    int32_t mode;                // 0: LeakyReLU(slope) on the raw score, 1: none (reference-literal mode)
};

struct EdgeGrad {                // GRAD: what the edge gradient needs on top of Recompute
    const float *Z;              // [nrows x ldz] Z_j of the task's row
    int64_t ldz;
    const float *t;              // [ncols x KH] t_i = <dOut_i, out_i>
    float *de;                   // [nnz x KH] entry-major, storage order of this (transposed) structure
    int32_t pw;                  // width of a partial / output row: F + heads rounded up to 4
};

struct Forward2 {                // FWD: the second output of the forward product
    float *C2;                   // [nrows x ldc2]: V in columns [0, F), C in [F, F + KH), zeros up to pw2
    int64_t ldc2;
    float *partial2;             // slot rows of pw2 floats (behind the F-wide slot rows of the first output)
    int32_t pw2;                 // F + heads rounded up to 4
};

}  // namespace
#endif
