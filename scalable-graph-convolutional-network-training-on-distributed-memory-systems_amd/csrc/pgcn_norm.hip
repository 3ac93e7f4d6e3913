// pgcn_norm.hip -- batch normalisation over ALL vertices of the graph, fused with the ReLU and the dropout keep function, for
// gfx950 (PGCN.py: _BatchNormReluDropout; include/pgcn_hip.h has the contract).
//
//   forward    sums = [sum_i x_ij, sum_i x_ij^2, rows]          pgcn_bn_colstats_f32       (two launches; then ONE float64 all-reduce)
//              mean, invstd, running statistics                  pgcn_bn_prepare_f32        (one block, reads the sums from memory)
//              y = keep ? max(0, g (x - mean) invstd + b) s : 0  pgcn_bn_relu_apply_f32     (one pass)
//   backward   sums = [sum_i g'_ij, sum_i g'_ij xh_ij], dg, db   pgcn_bn_backward_stats_f32 (two launches; then ONE float64 all-reduce)
//              dx = g invstd (g' - S1 / N - xh S2 / N)           pgcn_bn_relu_backward_f32  (one pass)
//   with g' = y > 0 ? g s : 0 (the saved output is its own mask) and xh = (x - mean) invstd.
//
// Layout, the same in every kernel: 256 threads; a thread owns FOUR consecutive columns (one float4), TPR = the power of two
// >= ceil(f / 4) threads span a row, 256 / TPR row groups walk a band of consecutive rows, four rows per thread in flight.  What
// belongs to a column (mean, invstd, gamma, beta, the column's share of the dropout hash, the global sums) is loaded or computed
// once per thread, before the row loop.  f <= 1024 is what 256 threads x 4 columns cover.  When f % 4 == 0 and every base and
// leading dimension keeps the rows 16-byte aligned the four columns move as one float4; otherwise the SAME thread moves them as
// four guarded scalars -- the same thread adds the same numbers in the same order, so both paths leave the same bits.
//
// Column sums: a block owns kStatRows consecutive rows; its threads add x and x^2 (g' and g' xh) in double registers, the row
// groups are folded through LDS by a fixed tree, and the block writes ONE partial record [2][f] of doubles to the work-space.
// The second launch gives each block 32 of the 2 f outputs: 8 groups of threads add the records b = group, group + 8, ... in
// that order, a fixed tree folds the 8 -- no floating-point atomics, the same input gives the same bits; at the Reddit shape
// (232 965 x 128) that is 456 bands and 8 blocks of the second level.  NaN and inf stay in their own column: no thread touches
// two columns' sums.  Raw pointers + a stream, no allocation, no synchronisation: graph-capturable.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"

#define PG_DROPOUT_FN __host__ __device__ __forceinline__
#include "../gemm/pgcn_dropout.h"

namespace {

constexpr int kThreads = 256;
constexpr int kStatRows = 512;     // rows of a band of the column-sum kernels (kernels.BN_STAT_ROWS restates it)
constexpr int kApplyRows = 128;    // rows of a block of the element-wise kernels
constexpr int kFinalCols = 32;     // outputs of a block of the second level
constexpr int kFinalGroups = kThreads / kFinalCols;
constexpr int kMaxF = 1024;

struct Geometry {
    int log2_tpr;     // threads per row = 1 << log2_tpr >= ceil(f / 4)
    bool vec;
};

struct Quad {
    float v[4];
};

template <bool VEC>
__device__ __forceinline__ Quad load_quad(const float *__restrict__ row, int c0, int f) {
    Quad q;
    if constexpr (VEC) {
        const float4 t = *reinterpret_cast<const float4 *>(row + c0);
        q.v[0] = t.x, q.v[1] = t.y, q.v[2] = t.z, q.v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) q.v[j] = c0 + j < f ? row[c0 + j] : 0.f;
    }
    return q;
}

template <bool VEC>
__device__ __forceinline__ void store_quad(float *__restrict__ row, int c0, int f, const Quad &q) {
    if constexpr (VEC) {
        *reinterpret_cast<float4 *>(row + c0) = make_float4(q.v[0], q.v[1], q.v[2], q.v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < f) row[c0 + j] = q.v[j];
    }
}

// a column's constant (0 beyond the last column: such a lane computes on zeros and stores nothing)
__device__ __forceinline__ Quad load_cols(const float *__restrict__ p, int c0, int f) {
    Quad q;
#pragma unroll
    for (int j = 0; j < 4; ++j) q.v[j] = c0 + j < f ? p[c0 + j] : 0.f;
    return q;
}

// The elements' arithmetic.  Contraction is off and the one fused multiply-add is written out, so that the float4 body and the
// scalar body cannot be compiled into different roundings.
__device__ __forceinline__ float bn_relu(float x, float mean, float a, float beta) {
#pragma clang fp contract(off)
    const float v = fmaf(a, x - mean, beta);
    return v < 0.f ? 0.f : v;                      // (NaN stays NaN: a poisoned column shows in its outputs)
}
__device__ __forceinline__ float masked_grad(float g, float y, float scale) {
#pragma clang fp contract(off)
    return y > 0.f ? g * scale : 0.f;
}
__device__ __forceinline__ float xhat(float x, float mean, float invstd) {
#pragma clang fp contract(off)
    return (x - mean) * invstd;
}

// Folds the 256 / TPR row groups of `acc` (8 doubles per thread) through LDS, k-major so that neighbouring threads touch
// neighbouring doubles; on return the threads of row group 0 hold the band's sums.
__device__ __forceinline__ void fold_row_groups(double (&acc)[8], double *sm, int tid, int log2_tpr) {
#pragma unroll
    for (int k = 0; k < 8; ++k) sm[k * kThreads + tid] = acc[k];
    for (int s = (kThreads >> log2_tpr) >> 1; s >= 1; s >>= 1) {
        __syncthreads();
        if ((tid >> log2_tpr) < s) {
#pragma unroll
            for (int k = 0; k < 8; ++k) sm[k * kThreads + tid] += sm[k * kThreads + tid + (s << log2_tpr)];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = sm[k * kThreads + tid];
}

__device__ __forceinline__ void write_partial(const double (&acc)[8], double *__restrict__ ws, int64_t band, int c0, int f) {
    double *rec = ws + band * 2 * (int64_t)f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (c0 + j < f) {
            rec[c0 + j] = acc[j];
            rec[f + c0 + j] = acc[4 + j];
        }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void colstats_kernel(const float *__restrict__ X, int64_t ldx, int64_t nrows, int f, int log2_tpr,
                                                            double *__restrict__ ws) {
#pragma clang fp contract(off)
    __shared__ double sm[8 * kThreads];
    const int tid = threadIdx.x, u = tid & ((1 << log2_tpr) - 1), rg = tid >> log2_tpr, ngroups = kThreads >> log2_tpr;
    const int c0 = 4 * u;
    const bool active = c0 < f;
    const int64_t r0 = (int64_t)blockIdx.x * kStatRows;
    const int64_t rend = r0 + kStatRows < nrows ? r0 + kStatRows : nrows;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (active) {
        for (int64_t r = r0 + rg; r < rend; r += 4 * (int64_t)ngroups) {
            Quad q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t rr = r + (int64_t)k * ngroups;
                if (rr < rend) q[k] = load_quad<VEC>(X + rr * ldx, c0, f);
                else q[k] = Quad{{0.f, 0.f, 0.f, 0.f}};
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double x = (double)q[k].v[j];
                    acc[j] += x;
                    acc[4 + j] += x * x;
                }
        }
    }
    fold_row_groups(acc, sm, tid, log2_tpr);
    if (rg == 0 && active) write_partial(acc, ws, blockIdx.x, c0, f);
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void backward_stats_kernel(const float *__restrict__ G, int64_t ldg, const float *__restrict__ Y,
                                                                  int64_t ldy, const float *__restrict__ X, int64_t ldx, int64_t nrows,
                                                                  int f, int log2_tpr, const float *__restrict__ mean,
                                                                  const float *__restrict__ invstd, float scale,
                                                                  double *__restrict__ ws) {
#pragma clang fp contract(off)
    __shared__ double sm[8 * kThreads];
    const int tid = threadIdx.x, u = tid & ((1 << log2_tpr) - 1), rg = tid >> log2_tpr, ngroups = kThreads >> log2_tpr;
    const int c0 = 4 * u;
    const bool active = c0 < f;
    const int64_t r0 = (int64_t)blockIdx.x * kStatRows;
    const int64_t rend = r0 + kStatRows < nrows ? r0 + kStatRows : nrows;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (active) {
        const Quad m = load_cols(mean, c0, f), is = load_cols(invstd, c0, f);
        for (int64_t r = r0 + rg; r < rend; r += 2 * (int64_t)ngroups) {
            Quad g[2], y[2], x[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int64_t rr = r + (int64_t)k * ngroups;
                if (rr < rend) {
                    g[k] = load_quad<VEC>(G + rr * ldg, c0, f);
                    y[k] = load_quad<VEC>(Y + rr * ldy, c0, f);
                    x[k] = load_quad<VEC>(X + rr * ldx, c0, f);
                } else {
                    g[k] = y[k] = x[k] = Quad{{0.f, 0.f, 0.f, 0.f}};        // (y = 0: masked, adds an exact zero)
                }
            }
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float gm = masked_grad(g[k].v[j], y[k].v[j], scale);
                    // xh in double here: S2 is a sum with cancellation, and the fp32 rounding of every xh would stay in it at
                    // full size (sum |g' xh| 2^-24, not |S2| 2^-24).  A masked element adds exact zeros whatever its x: an inf
                    // there must not turn 0 * inf into NaN.
                    const double xh = y[k].v[j] > 0.f ? ((double)x[k].v[j] - (double)m.v[j]) * (double)is.v[j] : 0.0;
                    acc[j] += (double)gm;
                    acc[4 + j] += (double)gm * xh;
                }
        }
    }
    fold_row_groups(acc, sm, tid, log2_tpr);
    if (rg == 0 && active) write_partial(acc, ws, blockIdx.x, c0, f);
}

// Second level: block b owns outputs 32 b .. 32 b + 31 of the 2 f; group g of its threads adds records g, g + 8, ... in that
// order, then the 8 groups are folded by a fixed tree.  out0 / out1 (optional): the first / second f sums as fp32 (dbeta and
// dgamma of the backward); count (optional): written behind the sums (the rows this rank owns, the forward's N after the
// all-reduce).
__global__ __launch_bounds__(kThreads) void finalize_kernel(const double *__restrict__ ws, int64_t nbands, int f, double *__restrict__ sums,
                                                            float *__restrict__ out0, float *__restrict__ out1, int want_count,
                                                            int64_t nrows) {
    __shared__ double sm[kThreads];
    const int tid = threadIdx.x, lane = tid & (kFinalCols - 1), grp = tid / kFinalCols;
    const int o = blockIdx.x * kFinalCols + lane;
    double acc = 0.0;
    if (o < 2 * f)
        for (int64_t b = grp; b < nbands; b += kFinalGroups) acc += ws[b * 2 * (int64_t)f + o];
    sm[tid] = acc;
    for (int s = kFinalGroups >> 1; s >= 1; s >>= 1) {
        __syncthreads();
        if (grp < s) sm[tid] += sm[tid + s * kFinalCols];
    }
    if (grp == 0 && o < 2 * f) {
        const double v = sm[tid];
        sums[o] = v;
        if (o < f) {
            if (out0) out0[o] = (float)v;
        } else if (out1) {
            out1[o - f] = (float)v;
        }
    }
    if (want_count && blockIdx.x == 0 && tid == 0) sums[2 * f] = (double)nrows;
}

__global__ __launch_bounds__(kThreads) void prepare_kernel(const double *__restrict__ sums, int f, double eps, double momentum, int training,
                                                           float *__restrict__ running_mean, float *__restrict__ running_var,
                                                           float *__restrict__ mean, float *__restrict__ invstd) {
#pragma clang fp contract(off)
    for (int c = threadIdx.x; c < f; c += kThreads) {
        if (!training) {
            mean[c] = running_mean[c];
            invstd[c] = (float)(1.0 / sqrt((double)running_var[c] + eps));
            continue;
        }
        const double N = sums[2 * f];
        if (!(N >= 1.0)) {                         // a graph without vertices: nothing to normalise with, nothing to record
            mean[c] = 0.f;
            invstd[c] = (float)(1.0 / sqrt(eps));
            continue;
        }
        const double m = sums[c] / N;
        double var = sums[f + c] / N - m * m;
        if (var < 0.0) var = 0.0;                  // (NaN stays NaN)
        mean[c] = (float)m;
        invstd[c] = (float)(1.0 / sqrt(var + eps));
        if (running_mean) running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * m);
        if (running_var) {
            const double unbiased = N > 1.0 ? var * (N / (N - 1.0)) : var;
            running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
        }
    }
}

struct DropArgs {
    const int64_t *row_ids;
    const int64_t *step;       // NULL: no dropout
    uint64_t seed;
    uint32_t layer, thr;
    float scale;
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void apply_kernel(const float *__restrict__ X, int64_t ldx, int64_t nrows, int f, int log2_tpr,
                                                         const float *__restrict__ mean, const float *__restrict__ invstd,
                                                         const float *__restrict__ gamma, const float *__restrict__ beta, DropArgs d,
                                                         float *__restrict__ Y, int64_t ldy) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, u = tid & ((1 << log2_tpr) - 1), rg = tid >> log2_tpr, ngroups = kThreads >> log2_tpr;
    const int c0 = 4 * u;
    if (c0 >= f) return;
    const int64_t r0 = (int64_t)blockIdx.x * kApplyRows;
    const int64_t rend = r0 + kApplyRows < nrows ? r0 + kApplyRows : nrows;
    const Quad m = load_cols(mean, c0, f), is = load_cols(invstd, c0, f), ga = load_cols(gamma, c0, f), be = load_cols(beta, c0, f);
    float a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = ga.v[j] * is.v[j];
    const bool drop = d.step != nullptr;
    uint64_t key = 0;
    uint32_t dcol[4] = {0, 0, 0, 0};
    if (drop) {
        key = dropout_key(d.seed, (uint64_t)d.step[0], d.layer);
#pragma unroll
        for (int j = 0; j < 4; ++j) dcol[j] = dropout_col(key, (uint32_t)(c0 + j));      // the column's share: once per column
    }
    for (int64_t r = r0 + rg; r < rend; r += 4 * (int64_t)ngroups) {
        Quad q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr < rend) q[k] = load_quad<VEC>(X + rr * ldx, c0, f);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr >= rend) break;
            Quad y;
#pragma unroll
            for (int j = 0; j < 4; ++j) y.v[j] = bn_relu(q[k].v[j], m.v[j], a[j], be.v[j]);
            if (drop) {
                const uint64_t grow = d.row_ids ? (uint64_t)d.row_ids[rr] : (uint64_t)rr;
                const uint32_t term = dropout_row(key, grow), hi = (uint32_t)(grow >> 32);
#pragma unroll
                for (int j = 0; j < 4; ++j) y.v[j] = dropout_u(dcol[j], term, hi) >= d.thr ? y.v[j] * d.scale : 0.f;
            }
            store_quad<VEC>(Y + rr * ldy, c0, f, y);
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void backward_kernel(const float *__restrict__ G, int64_t ldg, const float *__restrict__ Y, int64_t ldy,
                                                            const float *__restrict__ X, int64_t ldx, int64_t nrows, int f, int log2_tpr,
                                                            const float *__restrict__ mean, const float *__restrict__ invstd,
                                                            const float *__restrict__ gamma, const double *__restrict__ sums, double inv_n,
                                                            float scale, float *__restrict__ dX, int64_t lddx) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, u = tid & ((1 << log2_tpr) - 1), rg = tid >> log2_tpr, ngroups = kThreads >> log2_tpr;
    const int c0 = 4 * u;
    if (c0 >= f) return;
    const int64_t r0 = (int64_t)blockIdx.x * kApplyRows;
    const int64_t rend = r0 + kApplyRows < nrows ? r0 + kApplyRows : nrows;
    const Quad m = load_cols(mean, c0, f), is = load_cols(invstd, c0, f), ga = load_cols(gamma, c0, f);
    float a[4], c1[4], c2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[j] = ga.v[j] * is.v[j];
        c1[j] = c0 + j < f ? (float)(sums[c0 + j] * inv_n) : 0.f;
        c2[j] = c0 + j < f ? (float)(sums[f + c0 + j] * inv_n) : 0.f;
    }
    for (int64_t r = r0 + rg; r < rend; r += 2 * (int64_t)ngroups) {
        Quad g[2], y[2], x[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr < rend) {
                g[k] = load_quad<VEC>(G + rr * ldg, c0, f);
                y[k] = load_quad<VEC>(Y + rr * ldy, c0, f);
                x[k] = load_quad<VEC>(X + rr * ldx, c0, f);
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr >= rend) break;
            Quad o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float gm = masked_grad(g[k].v[j], y[k].v[j], scale);
                const float xh = xhat(x[k].v[j], m.v[j], is.v[j]);
                o.v[j] = a[j] * fmaf(-xh, c2[j], gm - c1[j]);
            }
            store_quad<VEC>(dX + rr * lddx, c0, f, o);
        }
    }
}

int log2_threads_per_row(int f) {
    const int quads = (f + 3) / 4;
    int l = 0;
    while ((1 << l) < quads) ++l;
    return l;
}

bool aligned16(const void *p) { return ((uintptr_t)p % 16) == 0; }
bool rows16(int64_t ld) { return ld % 4 == 0; }

int64_t bands(int64_t nrows) { return (nrows + kStatRows - 1) / kStatRows; }

// the checks every matrix operand shares; 0 = fine
int check_shape(const char *who, int64_t nrows, int32_t f) {
    if (nrows < 0 || f < 1) return pgcn_set_error2(PGCN_EINVAL, who, "nrows < 0 or f < 1");
    return 0;
}

}  // namespace

extern "C" int64_t pgcn_bn_colstats_ws_bytes(int64_t nrows, int32_t f) {
    if (nrows < 0 || f < 1 || f > kMaxF) return -1;
    const int64_t nb = bands(nrows);
    return (nb > 0 ? nb : 1) * 2 * (int64_t)f * (int64_t)sizeof(double);
}

extern "C" int pgcn_bn_colstats_f32(const float *X, int64_t ldx, int64_t nrows, int32_t f, double *sums, void *ws, int64_t ws_bytes,
                                    pgcn_stream_t stream) {
    if (int rc = check_shape("pgcn_bn_colstats_f32", nrows, f)) return rc;
    if (ldx < f) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_colstats_f32: ldx < f");
    if (!sums || !ws || (nrows > 0 && !X)) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_colstats_f32: null pointer");
    if ((uintptr_t)sums % 8 != 0 || (uintptr_t)ws % 8 != 0)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_colstats_f32: sums and ws must be 8-byte aligned");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_bn_colstats_f32: more than 1024 columns");
    if (ws_bytes < pgcn_bn_colstats_ws_bytes(nrows, f)) return pgcn_set_error(PGCN_ENOMEM, "pgcn_bn_colstats_f32: work-space too small");
    const int64_t nb = bands(nrows);
    const int l2 = log2_threads_per_row(f);
    hipStream_t s = (hipStream_t)stream;
    if (nb > 0) {
        const bool vec = f % 4 == 0 && rows16(ldx) && aligned16(X);
        if (vec)
            hipLaunchKernelGGL(colstats_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, s, X, ldx, nrows, (int)f, l2, (double *)ws);
        else
            hipLaunchKernelGGL(colstats_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, s, X, ldx, nrows, (int)f, l2, (double *)ws);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((2 * f + kFinalCols - 1) / kFinalCols)), dim3(kThreads), 0, s, (const double *)ws, nb,
                       (int)f, sums, (float *)nullptr, (float *)nullptr, 1, nrows);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_bn_backward_stats_f32(const float *G, int64_t ldg, const float *Y, int64_t ldy, const float *X, int64_t ldx,
                                          int64_t nrows, int32_t f, const float *mean, const float *invstd, float scale, double *sums,
                                          float *dgamma, float *dbeta, void *ws, int64_t ws_bytes, pgcn_stream_t stream) {
    if (int rc = check_shape("pgcn_bn_backward_stats_f32", nrows, f)) return rc;
    if (ldg < f || ldy < f || ldx < f) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_backward_stats_f32: a leading dimension is below f");
    if (!sums || !ws || !mean || !invstd || (nrows > 0 && (!G || !Y || !X)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_backward_stats_f32: null pointer");
    if ((uintptr_t)sums % 8 != 0 || (uintptr_t)ws % 8 != 0)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_backward_stats_f32: sums and ws must be 8-byte aligned");
    if (!(scale > 0.f && scale <= FLT_MAX)) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_backward_stats_f32: scale must be finite and > 0");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_bn_backward_stats_f32: more than 1024 columns");
    if (ws_bytes < pgcn_bn_colstats_ws_bytes(nrows, f))
        return pgcn_set_error(PGCN_ENOMEM, "pgcn_bn_backward_stats_f32: work-space too small");
    const int64_t nb = bands(nrows);
    const int l2 = log2_threads_per_row(f);
    hipStream_t s = (hipStream_t)stream;
    if (nb > 0) {
        const bool vec = f % 4 == 0 && rows16(ldg) && rows16(ldy) && rows16(ldx) && aligned16(G) && aligned16(Y) && aligned16(X);
        if (vec)
            hipLaunchKernelGGL(backward_stats_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, s, G, ldg, Y, ldy, X, ldx, nrows, (int)f, l2,
                               mean, invstd, scale, (double *)ws);
        else
            hipLaunchKernelGGL(backward_stats_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, s, G, ldg, Y, ldy, X, ldx, nrows, (int)f, l2,
                               mean, invstd, scale, (double *)ws);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((2 * f + kFinalCols - 1) / kFinalCols)), dim3(kThreads), 0, s, (const double *)ws, nb,
                       (int)f, sums, dbeta, dgamma, 0, nrows);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_bn_prepare_f32(const double *sums, int32_t f, double eps, double momentum, int32_t training, float *running_mean,
                                   float *running_var, float *mean, float *invstd, pgcn_stream_t stream) {
    if (f < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_prepare_f32: f < 1");
    if (!(eps > 0.0 && eps <= DBL_MAX)) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_prepare_f32: eps must be finite and > 0");
    if (!(momentum >= 0.0 && momentum <= 1.0)) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_prepare_f32: momentum must be in [0, 1]");
    if (!mean || !invstd) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_prepare_f32: null pointer");
    if (training ? !sums : (!running_mean || !running_var))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_prepare_f32: train mode needs the sums, eval mode the running statistics");
    if (training && (uintptr_t)sums % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_prepare_f32: sums must be 8-byte aligned");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_bn_prepare_f32: more than 1024 columns");
    hipLaunchKernelGGL(prepare_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, sums, (int)f, eps, momentum, (int)(training != 0),
                       running_mean, running_var, mean, invstd);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_bn_relu_apply_f32(const float *X, int64_t ldx, int64_t nrows, int32_t f, const float *mean, const float *invstd,
                                      const float *gamma, const float *beta, const int64_t *row_ids, uint64_t seed, const int64_t *step,
                                      uint32_t layer, uint32_t thr, float *Y, int64_t ldy, pgcn_stream_t stream) {
    if (int rc = check_shape("pgcn_bn_relu_apply_f32", nrows, f)) return rc;
    if (ldx < f || ldy < f) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_relu_apply_f32: a leading dimension is below f");
    if (!mean || !invstd || !gamma || !beta || (nrows > 0 && (!X || !Y)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_relu_apply_f32: null pointer");
    if (step && (uintptr_t)step % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_relu_apply_f32: step must be 8-byte aligned");
    if (row_ids && (uintptr_t)row_ids % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_relu_apply_f32: row_ids must be 8-byte aligned");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_bn_relu_apply_f32: more than 1024 columns");
    if (nrows == 0) return PGCN_OK;
    DropArgs d;
    d.row_ids = row_ids;
    d.step = thr > 0 ? step : nullptr;             // (thr == 0 keeps everything at scale 1: the path without dropout, bit for bit)
    d.seed = seed;
    d.layer = layer;
    d.thr = thr;
    d.scale = dropout_scale(thr);
    const int l2 = log2_threads_per_row(f);
    const int64_t nb = (nrows + kApplyRows - 1) / kApplyRows;
    const bool vec = f % 4 == 0 && rows16(ldx) && rows16(ldy) && aligned16(X) && aligned16(Y);
    if (vec)
        hipLaunchKernelGGL(apply_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, X, ldx, nrows, (int)f, l2, mean,
                           invstd, gamma, beta, d, Y, ldy);
    else
        hipLaunchKernelGGL(apply_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, X, ldx, nrows, (int)f, l2, mean,
                           invstd, gamma, beta, d, Y, ldy);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_bn_relu_backward_f32(const float *G, int64_t ldg, const float *Y, int64_t ldy, const float *X, int64_t ldx, int64_t nrows,
                                         int32_t f, const float *mean, const float *invstd, const float *gamma, const double *sums,
                                         int64_t N, float scale, float *dX, int64_t lddx, pgcn_stream_t stream) {
    if (int rc = check_shape("pgcn_bn_relu_backward_f32", nrows, f)) return rc;
    if (ldg < f || ldy < f || ldx < f || lddx < f)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_relu_backward_f32: a leading dimension is below f");
    if (!mean || !invstd || !gamma || !sums || (nrows > 0 && (!G || !Y || !X || !dX)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_relu_backward_f32: null pointer");
    if ((uintptr_t)sums % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_relu_backward_f32: sums must be 8-byte aligned");
    if (N < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_relu_backward_f32: N < 1");
    if (!(scale > 0.f && scale <= FLT_MAX)) return pgcn_set_error(PGCN_EINVAL, "pgcn_bn_relu_backward_f32: scale must be finite and > 0");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_bn_relu_backward_f32: more than 1024 columns");
    if (nrows == 0) return PGCN_OK;
    const int l2 = log2_threads_per_row(f);
    const int64_t nb = (nrows + kApplyRows - 1) / kApplyRows;
    const bool vec = f % 4 == 0 && rows16(ldg) && rows16(ldy) && rows16(ldx) && rows16(lddx) && aligned16(G) && aligned16(Y) &&
                     aligned16(X) && aligned16(dX);
    if (vec)
        hipLaunchKernelGGL(backward_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, G, ldg, Y, ldy, X, ldx, nrows,
                           (int)f, l2, mean, invstd, gamma, sums, 1.0 / (double)N, scale, dX, lddx);
    else
        hipLaunchKernelGGL(backward_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, G, ldg, Y, ldy, X, ldx, nrows,
                           (int)f, l2, mean, invstd, gamma, sums, 1.0 / (double)N, scale, dX, lddx);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}
