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
// The layout of the kernels, the dropout pieces and the deterministic column sums (partial records [2][f] here) are those of
// pgcn_rowband.h.  Raw pointers + a stream, no allocation, no synchronisation: graph-capturable.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"
#include "pgcn_rowband.h"

namespace {

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

template <bool VEC>
__global__ __launch_bounds__(kThreads) void colstats_kernel(const float *__restrict__ X, int64_t ldx, int64_t nrows, int f, int log2_tpr,
                                                            double *__restrict__ ws) {
#pragma clang fp contract(off)
    __shared__ double sm[8 * kThreads];
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kSumRows, nrows);
    const bool active = c0 < f;
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
    fold_row_groups(acc, sm, log2_tpr);
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
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kSumRows, nrows);
    const bool active = c0 < f;
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
    fold_row_groups(acc, sm, log2_tpr);
    if (rg == 0 && active) write_partial(acc, ws, blockIdx.x, c0, f);
}

// Second level of the 2 f sums.  out0 / out1 (optional): the first / second f sums as fp32 (dbeta and dgamma of the backward);
// count (optional): written behind the sums (the rows this rank owns, the forward's N after the all-reduce).
__global__ __launch_bounds__(kThreads) void finalize_kernel(const double *__restrict__ ws, int64_t nbands, int f, double *__restrict__ sums,
                                                            float *__restrict__ out0, float *__restrict__ out1, int want_count,
                                                            int64_t nrows) {
    final_sum<2>(ws, nbands, f, [=](int o, double v) {
        sums[o] = v;
        if (o < f) {
            if (out0) out0[o] = (float)v;
        } else if (out1) {
            out1[o - f] = (float)v;
        }
    });
    if (want_count && blockIdx.x == 0 && threadIdx.x == 0) sums[2 * f] = (double)nrows;
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

template <bool VEC>
__global__ __launch_bounds__(kThreads) void apply_kernel(const float *__restrict__ X, int64_t ldx, int64_t nrows, int f, int log2_tpr,
                                                         const float *__restrict__ mean, const float *__restrict__ invstd,
                                                         const float *__restrict__ gamma, const float *__restrict__ beta, DropArgs d,
                                                         float *__restrict__ Y, int64_t ldy) {
#pragma clang fp contract(off)
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kApplyRows, nrows);
    if (c0 >= f) return;
    const Quad m = load_cols(mean, c0, f), is = load_cols(invstd, c0, f), ga = load_cols(gamma, c0, f), be = load_cols(beta, c0, f);
    float a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = ga.v[j] * is.v[j];
    const DropCols dc = drop_cols(d.step, d.seed, d.layer, c0);
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
            if (dc.on) {
                const DropRow dr = drop_row(d.row_ids, dc, rr);
#pragma unroll
                for (int j = 0; j < 4; ++j) y.v[j] = drop_keep(dc, dr, j, d.thr) ? y.v[j] * d.scale : 0.f;
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
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kApplyRows, nrows);
    if (c0 >= f) return;
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

// the checks every matrix operand shares; 0 = fine
int check_shape(const char *who, int64_t nrows, int32_t f) {
    if (nrows < 0 || f < 1) return pgcn_set_error2(PGCN_EINVAL, who, "nrows < 0 or f < 1");
    return 0;
}

}  // namespace

extern "C" int64_t pgcn_bn_colstats_ws_bytes(int64_t nrows, int32_t f) { return ws_bytes(nrows, f, 2); }

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
        launch(vec ? colstats_kernel<true> : colstats_kernel<false>, nb, s, X, ldx, nrows, f, l2, ws);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    launch(finalize_kernel, final_blocks(2 * f), s, ws, nb, f, sums, nullptr, nullptr, 1, nrows);
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
        launch(vec ? backward_stats_kernel<true> : backward_stats_kernel<false>, nb, s, G, ldg, Y, ldy, X, ldx, nrows, f, l2, mean, invstd,
               scale, ws);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    launch(finalize_kernel, final_blocks(2 * f), s, ws, nb, f, sums, dbeta, dgamma, 0, nrows);
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
    const bool vec = f % 4 == 0 && rows16(ldx) && rows16(ldy) && aligned16(X) && aligned16(Y);
    launch(vec ? apply_kernel<true> : apply_kernel<false>, apply_blocks(nrows), (hipStream_t)stream, X, ldx, nrows, f,
           log2_threads_per_row(f), mean, invstd, gamma, beta, drop_args(row_ids, seed, step, layer, thr), Y, ldy);
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
    const bool vec = f % 4 == 0 && rows16(ldg) && rows16(ldy) && rows16(ldx) && rows16(lddx) && aligned16(G) && aligned16(Y) &&
                     aligned16(X) && aligned16(dX);
    launch(vec ? backward_kernel<true> : backward_kernel<false>, apply_blocks(nrows), (hipStream_t)stream, G, ldg, Y, ldy, X, ldx, nrows, f,
           log2_threads_per_row(f), mean, invstd, gamma, sums, 1.0 / (double)N, scale, dX, lddx);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}
