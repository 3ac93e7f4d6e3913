// pgcn_layernorm.hip -- layer normalisation of ONE VERTEX over its own features, fused with the ReLU, the dropout keep function and a
// residual link, for gfx950 (PGCN.py: _LayerNormReluDropout; include/pgcn_hip.h has the contract).
//
//   forward    mean_i = sum_j x / f;  var_i = sum_j (x - mean_i)^2 / f;  rstd_i = 1 / sqrt(var_i + eps)     (two passes, in registers)
//              xh = (x - mean_i) rstd_i;  t = fma(gamma_j, xh, beta_j);  d = keep ? max(0, t) s : 0;  y = R ? R + d : d
//              bit (i, j) = keep and t > 0                                          pgcn_ln_relu_forward_f32   (one launch)
//   backward   g' = bit ? g s : 0;  gh = g' gamma_j;  c1 = sum_j gh / f;  c2 = sum_j gh xh / f
//              dx = rstd_i ((gh - c1) - xh c2);  dbeta_j = float(sum_i g');  dgamma_j = float(sum_i g' xh)
//                                                                                   pgcn_ln_relu_backward_f32  (one pass + the second
//                                                                                   level of the column sums)
// Row-local: no collective, no dependence on the partition.  With a residual added y > 0 no longer says which elements survived, so
// the forward leaves 1 bit per element (the sign-mask layout of include/pgcn_gemm.h) and the backward reads g, x and the bits: no y.
//
// The layout of pgcn_rowband.h, two rows per thread in flight; both paths leave the same bits PROVIDED nothing is contracted:
// csrc/build.sh compiles this file with -ffp-contract=off (the pragmas below are not honoured under the command line's
// -ffp-contract=fast; they stay as a statement of intent), so the only fused operations are the one written fmaf and the expansions
// of division and square root.
//
// Row sums (fp32): a thread adds its quad ((q0 + q1) + q2) + q3, columns at and beyond f as zeros; then an xor butterfly over the
// row's aligned group of TPR lanes (TPR <= 64: inside one wave; addition commutes, so every lane ends with the same bits); TPR = 128
// or 256: the butterfly over the whole wave, lane 0 of each wave leaves its partial in LDS, every thread adds its row's 2 or 4
// partials as (p0 + p1) [+ (p2 + p3)].  Nothing in that tree knows the row's index, the block or nrows: a row's results are a
// function of the row.  EVERY thread of a block walks every iteration (rows beyond the band and columns beyond f compute on zeros and
// store nothing): the shuffles and the barriers are never divergent.
//
// Column sums of the backward (g' and g' xh, partial records [2][f]) and the dropout pieces: those of pgcn_rowband.h.  A masked-out
// element adds exact zeros whatever its x.  Raw pointers + a stream, no allocation, no synchronisation: graph-capturable.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"
#include "pgcn_rowband.h"

namespace {

constexpr int kWaves = kThreads / 64;
constexpr int kInFlight = 2;       // rows a thread holds at once

__device__ __forceinline__ float quad_sum(const float (&e)[4]) {
#pragma clang fp contract(off)
    return ((e[0] + e[1]) + e[2]) + e[3];
}

// v[k] <- the sum of v[k] over the tpr threads of this thread's row, k < NV, the same bits in every one of them.  CROSS (tpr = 128 or
// 256): `sm` holds 2 x NV x kWaves floats, `phase` picks the half -- successive calls alternate, so that ONE barrier per call is
// enough (a wave that runs ahead writes the other half; the half it will write after that was last read before the barrier between).
template <int NV, bool CROSS>
__device__ __forceinline__ void row_sums(float (&v)[NV], int tpr, float *sm, int phase, int tid) {
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        if (m < tpr) {                               // (uniform over the block)
#pragma unroll
            for (int k = 0; k < NV; ++k) v[k] += __shfl_xor(v[k], m, 64);
        }
    }
    if constexpr (CROSS) {
        const int wave = tid >> 6;
        float *s = sm + (phase & 1) * NV * kWaves;
        if ((tid & 63) == 0) {
#pragma unroll
            for (int k = 0; k < NV; ++k) s[k * kWaves + wave] = v[k];
        }
        __syncthreads();
        if (tpr == kThreads) {
#pragma unroll
            for (int k = 0; k < NV; ++k) v[k] = (s[k * kWaves] + s[k * kWaves + 1]) + (s[k * kWaves + 2] + s[k * kWaves + 3]);
        } else {
            const int w0 = wave & ~1;
#pragma unroll
            for (int k = 0; k < NV; ++k) v[k] = s[k * kWaves + w0] + s[k * kWaves + w0 + 1];
        }
    }
}

template <bool VEC, bool CROSS>
__global__ __launch_bounds__(kThreads) void forward_kernel(const float *X, int64_t ldx, int64_t nrows, int f, int log2_tpr,
                                                           const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                           const float *R, int64_t ldr, DropArgs d, float *Y, int64_t ldy,
                                                           float *__restrict__ mean, float *__restrict__ rstd, int32_t *__restrict__ mask) {
#pragma clang fp contract(off)
    __shared__ float sm[2 * kInFlight * kWaves];
    const int tid = threadIdx.x;
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kApplyRows, nrows);
    const bool active = c0 < f;
    const int mw = (f + 31) >> 5;
    const float ff = (float)f;
    const Quad ga = load_cols(gamma, c0, f), be = load_cols(beta, c0, f);
    const DropCols dc = drop_cols(d.step, d.seed, d.layer, c0);
    for (int64_t base = r0; base < rend; base += kInFlight * (int64_t)ngroups) {          // (uniform over the block)
        int64_t rr[kInFlight];
        bool ok[kInFlight];
        Quad q[kInFlight];
        float s[kInFlight], mu[kInFlight], rs[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            rr[k] = base + (int64_t)k * ngroups + rg;
            ok[k] = rr[k] < rend && active;
            if (ok[k]) q[k] = load_quad<VEC>(X + rr[k] * ldx, c0, f);
            else q[k] = Quad{{0.f, 0.f, 0.f, 0.f}};
            s[k] = quad_sum(q[k].v);
        }
        row_sums<kInFlight, CROSS>(s, tpr, sm, 0, tid);
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            mu[k] = s[k] / ff;
            float e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float c = q[k].v[j] - mu[k];
                e[j] = c0 + j < f ? c * c : 0.f;
            }
            s[k] = quad_sum(e);
        }
        row_sums<kInFlight, CROSS>(s, tpr, sm, 1, tid);
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            rs[k] = 1.0f / sqrtf(s[k] / ff + eps);
            Quad y;
            uint32_t bits = 0;
            if (ok[k]) {
                const DropRow dr = dc.on ? drop_row(d.row_ids, dc, rr[k]) : DropRow{0, 0};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float xh = (q[k].v[j] - mu[k]) * rs[k];
                    const float t = fmaf(ga.v[j], xh, be.v[j]);
                    float v = t < 0.f ? 0.f : t;                                          // (NaN stays NaN)
                    bool keep = true;
                    if (dc.on) {
                        keep = drop_keep(dc, dr, j, d.thr);
                        v = keep ? v * d.scale : 0.f;
                    }
                    if (keep && t > 0.f && c0 + j < f) bits |= 1u << j;
                    y.v[j] = v;
                }
                if (R) {
                    const Quad r = load_quad<VEC>(R + rr[k] * ldr, c0, f);
#pragma unroll
                    for (int j = 0; j < 4; ++j) y.v[j] = r.v[j] + y.v[j];
                }
                store_quad<VEC>(Y + rr[k] * ldy, c0, f, y);
                if (mean && u == 0) {
                    mean[rr[k]] = mu[k];
                    rstd[rr[k]] = rs[k];
                }
            }
            if (mask) {                                                                   // (uniform: every lane takes the shuffles)
                uint32_t word = bits << (4 * (u & 7));                                    // 8 neighbouring threads hold one word
#pragma unroll
                for (int m = 1; m < 8; m <<= 1)
                    if (m < tpr) word |= (uint32_t)__shfl_xor((int)word, m, 64);
                if (ok[k] && (u & 7) == 0) mask[rr[k] * mw + (u >> 3)] = (int32_t)word;
            }
        }
    }
}

template <bool VEC, bool CROSS, bool SUMS>
__global__ __launch_bounds__(kThreads) void backward_kernel(const float *G, int64_t ldg, const float *X, int64_t ldx, int64_t nrows, int f,
                                                            int log2_tpr, const float *__restrict__ mean, const float *__restrict__ rstd,
                                                            const float *__restrict__ gamma, const int32_t *__restrict__ mask, float scale,
                                                            float *dX, int64_t lddx, double *__restrict__ ws) {
#pragma clang fp contract(off)
    __shared__ float sm[2 * 2 * kInFlight * kWaves];
    __shared__ double smd[SUMS ? 8 * kThreads : 1];
    const int tid = threadIdx.x;
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kSumRows, nrows);
    const bool active = c0 < f;
    const int mw = (f + 31) >> 5;
    const float ff = (float)f;
    const Quad ga = load_cols(gamma, c0, f);
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int phase = 0;
    for (int64_t base = r0; base < rend; base += kInFlight * (int64_t)ngroups, ++phase) {  // (uniform over the block)
        int64_t rr[kInFlight];
        bool ok[kInFlight];
        Quad gh[kInFlight], xh[kInFlight];
        float rs[kInFlight], s[2 * kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            rr[k] = base + (int64_t)k * ngroups + rg;
            ok[k] = rr[k] < rend && active;
            Quad g, x;
            uint32_t bits = 0;
            float mu = 0.f;
            rs[k] = 0.f;
            if (ok[k]) {
                g = load_quad<VEC>(G + rr[k] * ldg, c0, f);
                x = load_quad<VEC>(X + rr[k] * ldx, c0, f);
                bits = ((uint32_t)mask[rr[k] * mw + (c0 >> 5)] >> (c0 & 31)) & 15u;
                mu = mean[rr[k]];
                rs[k] = rstd[rr[k]];
            } else {
                g = x = Quad{{0.f, 0.f, 0.f, 0.f}};
            }
            float p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool bit = (bits >> j) & 1u;
                const float gm = bit ? g.v[j] * scale : 0.f;
                xh[k].v[j] = (x.v[j] - mu) * rs[k];
                gh[k].v[j] = gm * ga.v[j];
                p[j] = gh[k].v[j] * xh[k].v[j];
                if constexpr (SUMS) {
                    // a masked-out element adds exact zeros whatever its x: a NaN or inf there must not reach the column's sums
                    acc[j] += (double)gm;
                    acc[4 + j] += bit ? (double)gm * (double)xh[k].v[j] : 0.0;
                }
            }
            s[2 * k] = quad_sum(gh[k].v);
            s[2 * k + 1] = quad_sum(p);
        }
        row_sums<2 * kInFlight, CROSS>(s, tpr, sm, phase, tid);
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            if (!ok[k]) continue;
            const float c1 = s[2 * k] / ff, c2 = s[2 * k + 1] / ff;
            Quad o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float w = xh[k].v[j] * c2;
                o.v[j] = rs[k] * ((gh[k].v[j] - c1) - w);
            }
            store_quad<VEC>(dX + rr[k] * lddx, c0, f, o);
        }
    }
    if constexpr (SUMS) {
        fold_row_groups(acc, smd, log2_tpr);
        if (rg == 0 && active) write_partial(acc, ws, blockIdx.x, c0, f);
    }
}

// Second level of the 2 f sums: the first f are dbeta, the second f dgamma.  No record: zeros.
__global__ __launch_bounds__(kThreads) void finalize_kernel(const double *__restrict__ ws, int64_t nbands, int f, float *__restrict__ dbeta,
                                                            float *__restrict__ dgamma) {
    final_sum<2>(ws, nbands, f, [=](int o, double v) {
        if (o < f) dbeta[o] = (float)v;
        else dgamma[o - f] = (float)v;
    });
}

}  // namespace

extern "C" int64_t pgcn_ln_ws_bytes(int64_t nrows, int32_t f) { return ws_bytes(nrows, f, 2); }

extern "C" int pgcn_ln_relu_forward_f32(const float *X, int64_t ldx, int64_t nrows, int32_t f, const float *gamma, const float *beta,
                                        double eps, const float *R, int64_t ldr, const int64_t *row_ids, uint64_t seed,
                                        const int64_t *step, uint32_t layer, uint32_t thr, float *Y, int64_t ldy, float *mean, float *rstd,
                                        int32_t *mask, pgcn_stream_t stream) {
    if (nrows < 0 || f < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_forward_f32: nrows < 0 or f < 1");
    if (ldx < f || ldy < f || (R && ldr < f)) return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_forward_f32: a leading dimension is below f");
    if (!gamma || !beta || (nrows > 0 && (!X || !Y))) return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_forward_f32: null pointer");
    if (!(eps > 0.0 && eps <= DBL_MAX) || !((float)eps > 0.f && (float)eps <= FLT_MAX))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_forward_f32: eps must be finite and > 0");
    if (step && (uintptr_t)step % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_forward_f32: step must be 8-byte aligned");
    if (row_ids && (uintptr_t)row_ids % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_forward_f32: row_ids must be 8-byte aligned");
    if (mask && (uintptr_t)mask % 4 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_forward_f32: mask must be 4-byte aligned");
    if ((mean != nullptr) != (rstd != nullptr) || (mean != nullptr) != (mask != nullptr))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_forward_f32: mean, rstd and mask go together (all three or none)");
    if (Y && Y == R && ldy != ldr) return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_forward_f32: in place (Y == R) needs ldy == ldr");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_ln_relu_forward_f32: more than 1024 columns");
    if (nrows == 0) return PGCN_OK;
    const int l2 = log2_threads_per_row(f);
    const bool vec = f % 4 == 0 && rows16(ldx) && rows16(ldy) && aligned16(X) && aligned16(Y) && (!R || (rows16(ldr) && aligned16(R)));
    const bool cross = l2 > 6;
    launch(cross ? (vec ? forward_kernel<true, true> : forward_kernel<false, true>) : (vec ? forward_kernel<true, false> : forward_kernel<false, false>),
           apply_blocks(nrows), (hipStream_t)stream, X, ldx, nrows, f, l2, gamma, beta, eps, R, ldr, drop_args(row_ids, seed, step, layer, thr),
           Y, ldy, mean, rstd, mask);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_ln_relu_backward_f32(const float *G, int64_t ldg, const float *X, int64_t ldx, int64_t nrows, int32_t f,
                                         const float *mean, const float *rstd, const float *gamma, const int32_t *mask, float scale,
                                         float *dX, int64_t lddx, float *dgamma, float *dbeta, void *ws, int64_t ws_bytes,
                                         pgcn_stream_t stream) {
    if (nrows < 0 || f < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_backward_f32: nrows < 0 or f < 1");
    if (ldg < f || ldx < f || lddx < f) return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_backward_f32: a leading dimension is below f");
    if (!gamma || (nrows > 0 && (!G || !X || !dX || !mean || !rstd || !mask)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_backward_f32: null pointer");
    if ((dgamma != nullptr) != (dbeta != nullptr))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_backward_f32: dgamma and dbeta go together (both or neither)");
    const bool sums = dgamma != nullptr;
    if (sums && !ws) return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_backward_f32: dgamma and dbeta need a work-space");
    if (sums && (uintptr_t)ws % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_backward_f32: ws must be 8-byte aligned");
    if (mask && (uintptr_t)mask % 4 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_backward_f32: mask must be 4-byte aligned");
    if (!(scale > 0.f && scale <= FLT_MAX)) return pgcn_set_error(PGCN_EINVAL, "pgcn_ln_relu_backward_f32: scale must be finite and > 0");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_ln_relu_backward_f32: more than 1024 columns");
    if (sums && ws_bytes < pgcn_ln_ws_bytes(nrows, f)) return pgcn_set_error(PGCN_ENOMEM, "pgcn_ln_relu_backward_f32: work-space too small");
    const int64_t nb = bands(nrows);
    const int l2 = log2_threads_per_row(f);
    hipStream_t s = (hipStream_t)stream;
    if (nb > 0) {
        const bool vec = f % 4 == 0 && rows16(ldg) && rows16(ldx) && rows16(lddx) && aligned16(G) && aligned16(X) && aligned16(dX);
        const bool cross = l2 > 6;
        launch(sums ? (cross ? (vec ? backward_kernel<true, true, true> : backward_kernel<false, true, true>)
                             : (vec ? backward_kernel<true, false, true> : backward_kernel<false, false, true>))
                    : (cross ? (vec ? backward_kernel<true, true, false> : backward_kernel<false, true, false>)
                             : (vec ? backward_kernel<true, false, false> : backward_kernel<false, false, false>)),
               nb, s, G, ldg, X, ldx, nrows, f, l2, mean, rstd, gamma, mask, scale, dX, lddx, sums ? ws : nullptr);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    if (sums) {
        launch(finalize_kernel, final_blocks(2 * f), s, ws, nb, f, dbeta, dgamma);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    return PGCN_OK;
}
