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
// Layout as in pgcn_norm.hip: 256 threads; a thread owns FOUR consecutive columns, TPR = the power of two >= ceil(f / 4) threads span
// a row, 256 / TPR row groups walk consecutive rows, two rows per thread in flight.  f <= 1024.  One float4 per thread and row when
// f % 4 == 0 and every base and leading dimension keeps the rows 16-byte aligned, four guarded scalars otherwise: the same thread does
// the same arithmetic in the same order, so both paths leave the same bits -- PROVIDED nothing is contracted: csrc/build.sh compiles
// this file with -ffp-contract=off (the pragmas below are not honoured under the command line's -ffp-contract=fast; they stay as a
// statement of intent), so the only fused operations are the one written fmaf and the expansions of division and square root.
//
// Row sums (fp32): a thread adds its quad ((q0 + q1) + q2) + q3, columns at and beyond f as zeros; then an xor butterfly over the
// row's aligned group of TPR lanes (TPR <= 64: inside one wave; addition commutes, so every lane ends with the same bits); TPR = 128
// or 256: the butterfly over the whole wave, lane 0 of each wave leaves its partial in LDS, every thread adds its row's 2 or 4
// partials as (p0 + p1) [+ (p2 + p3)].  Nothing in that tree knows the row's index, the block or nrows: a row's results are a
// function of the row.  EVERY thread of a block walks every iteration (rows beyond the band and columns beyond f compute on zeros and
// store nothing): the shuffles and the barriers are never divergent.
//
// Column sums of the backward: the scheme of pgcn_norm.hip -- a block owns kBandRows consecutive rows, its threads add g' and g' xh in
// double registers, the row groups are folded through LDS by a fixed tree, the block writes ONE partial record [2][f] of doubles; the
// second launch gives each block 32 of the 2 f outputs, 8 groups of threads add the records b = group, group + 8, ... in that order
// and a fixed tree folds the 8.  No floating-point atomics.  A masked-out element adds exact zeros whatever its x.
// Raw pointers + a stream, no allocation, no synchronisation: graph-capturable.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"

#define PG_DROPOUT_FN __host__ __device__ __forceinline__
#include "../gemm/pgcn_dropout.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBandRows = 512;     // rows of a block of the backward (kernels.LN_STAT_ROWS restates it)
constexpr int kApplyRows = 128;    // rows of a block of the forward
constexpr int kInFlight = 2;       // rows a thread holds at once
constexpr int kFinalCols = 32;     // outputs of a block of the second level
constexpr int kFinalGroups = kThreads / kFinalCols;
constexpr int kMaxF = 1024;

struct Quad {
    float v[4];
};

// (no __restrict__ on the matrices: Y may be R itself; a thread reads its own elements before it writes them)
template <bool VEC>
__device__ __forceinline__ Quad load_quad(const float *row, int c0, int f) {
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
__device__ __forceinline__ void store_quad(float *row, int c0, int f, const Quad &q) {
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

struct DropArgs {
    const int64_t *row_ids;
    const int64_t *step;       // NULL: no dropout
    uint64_t seed;
    uint32_t layer, thr;
    float scale;
};

template <bool VEC, bool CROSS>
__global__ __launch_bounds__(kThreads) void forward_kernel(const float *X, int64_t ldx, int64_t nrows, int f, int log2_tpr,
                                                           const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                           const float *R, int64_t ldr, DropArgs d, float *Y, int64_t ldy,
                                                           float *__restrict__ mean, float *__restrict__ rstd, int32_t *__restrict__ mask) {
#pragma clang fp contract(off)
    __shared__ float sm[2 * kInFlight * kWaves];
    const int tid = threadIdx.x, tpr = 1 << log2_tpr, u = tid & (tpr - 1), rg = tid >> log2_tpr, ngroups = kThreads >> log2_tpr;
    const int c0 = 4 * u;
    const bool active = c0 < f;
    const int mw = (f + 31) >> 5;
    const float ff = (float)f;
    const int64_t r0 = (int64_t)blockIdx.x * kApplyRows;
    const int64_t rend = r0 + kApplyRows < nrows ? r0 + kApplyRows : nrows;
    const Quad ga = load_cols(gamma, c0, f), be = load_cols(beta, c0, f);
    const bool drop = d.step != nullptr;
    uint64_t key = 0;
    uint32_t dcol[4] = {0, 0, 0, 0};
    if (drop) {
        key = dropout_key(d.seed, (uint64_t)d.step[0], d.layer);
#pragma unroll
        for (int j = 0; j < 4; ++j) dcol[j] = dropout_col(key, (uint32_t)(c0 + j));      // the column's share: once per thread
    }
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
                uint32_t term = 0, hi = 0;
                if (drop) {
                    const uint64_t grow = d.row_ids ? (uint64_t)d.row_ids[rr[k]] : (uint64_t)rr[k];
                    term = dropout_row(key, grow), hi = (uint32_t)(grow >> 32);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float xh = (q[k].v[j] - mu[k]) * rs[k];
                    const float t = fmaf(ga.v[j], xh, be.v[j]);
                    float v = t < 0.f ? 0.f : t;                                          // (NaN stays NaN)
                    bool keep = true;
                    if (drop) {
                        keep = dropout_u(dcol[j], term, hi) >= d.thr;
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
    const int tid = threadIdx.x, tpr = 1 << log2_tpr, u = tid & (tpr - 1), rg = tid >> log2_tpr, ngroups = kThreads >> log2_tpr;
    const int c0 = 4 * u;
    const bool active = c0 < f;
    const int mw = (f + 31) >> 5;
    const float ff = (float)f;
    const int64_t r0 = (int64_t)blockIdx.x * kBandRows;
    const int64_t rend = r0 + kBandRows < nrows ? r0 + kBandRows : nrows;
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
        // fold the 256 / TPR row groups through LDS by a fixed tree, k-major: neighbouring threads touch neighbouring doubles
#pragma unroll
        for (int k = 0; k < 8; ++k) smd[k * kThreads + tid] = acc[k];
        for (int st = ngroups >> 1; st >= 1; st >>= 1) {
            __syncthreads();
            if (rg < st) {
#pragma unroll
                for (int k = 0; k < 8; ++k) smd[k * kThreads + tid] += smd[k * kThreads + tid + (st << log2_tpr)];
            }
        }
        __syncthreads();
        if (rg == 0 && active) {
            double *rec = ws + (int64_t)blockIdx.x * 2 * (int64_t)f;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c0 + j < f) {
                    rec[c0 + j] = smd[j * kThreads + tid];
                    rec[f + c0 + j] = smd[(4 + j) * kThreads + tid];
                }
        }
    }
}

// Second level: block b owns outputs 32 b .. 32 b + 31 of the 2 f; group g of its threads adds records g, g + 8, ... in that
// order, then the 8 groups are folded by a fixed tree.  The first f sums are dbeta, the second f dgamma.  No record: zeros.
__global__ __launch_bounds__(kThreads) void finalize_kernel(const double *__restrict__ ws, int64_t nbands, int f, float *__restrict__ dbeta,
                                                            float *__restrict__ dgamma) {
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
        if (o < f) dbeta[o] = (float)sm[tid];
        else dgamma[o - f] = (float)sm[tid];
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
int64_t bands(int64_t nrows) { return (nrows + kBandRows - 1) / kBandRows; }

template <bool VEC, bool CROSS>
void launch_forward(int64_t nb, hipStream_t s, const float *X, int64_t ldx, int64_t nrows, int f, int l2, const float *gamma,
                    const float *beta, float eps, const float *R, int64_t ldr, const DropArgs &d, float *Y, int64_t ldy, float *mean,
                    float *rstd, int32_t *mask) {
    hipLaunchKernelGGL((forward_kernel<VEC, CROSS>), dim3((unsigned)nb), dim3(kThreads), 0, s, X, ldx, nrows, f, l2, gamma, beta, eps, R, ldr,
                       d, Y, ldy, mean, rstd, mask);
}

template <bool VEC, bool CROSS, bool SUMS>
void launch_backward(int64_t nb, hipStream_t s, const float *G, int64_t ldg, const float *X, int64_t ldx, int64_t nrows, int f, int l2,
                     const float *mean, const float *rstd, const float *gamma, const int32_t *mask, float scale, float *dX, int64_t lddx,
                     double *ws) {
    hipLaunchKernelGGL((backward_kernel<VEC, CROSS, SUMS>), dim3((unsigned)nb), dim3(kThreads), 0, s, G, ldg, X, ldx, nrows, f, l2, mean,
                       rstd, gamma, mask, scale, dX, lddx, ws);
}

}  // namespace

extern "C" int64_t pgcn_ln_ws_bytes(int64_t nrows, int32_t f) {
    if (nrows < 0 || f < 1 || f > kMaxF) return -1;
    const int64_t nb = bands(nrows);
    return (nb > 0 ? nb : 1) * 2 * (int64_t)f * (int64_t)sizeof(double);
}

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
    DropArgs d;
    d.row_ids = row_ids;
    d.step = thr > 0 ? step : nullptr;             // (thr == 0 keeps everything at scale 1: the path without dropout, bit for bit)
    d.seed = seed;
    d.layer = layer;
    d.thr = thr;
    d.scale = dropout_scale(thr);
    const int l2 = log2_threads_per_row(f);
    const int64_t nb = (nrows + kApplyRows - 1) / kApplyRows;
    const bool vec = f % 4 == 0 && rows16(ldx) && rows16(ldy) && aligned16(X) && aligned16(Y) && (!R || (rows16(ldr) && aligned16(R)));
    const bool cross = l2 > 6;
    hipStream_t s = (hipStream_t)stream;
    if (vec && cross) launch_forward<true, true>(nb, s, X, ldx, nrows, f, l2, gamma, beta, (float)eps, R, ldr, d, Y, ldy, mean, rstd, mask);
    else if (vec) launch_forward<true, false>(nb, s, X, ldx, nrows, f, l2, gamma, beta, (float)eps, R, ldr, d, Y, ldy, mean, rstd, mask);
    else if (cross) launch_forward<false, true>(nb, s, X, ldx, nrows, f, l2, gamma, beta, (float)eps, R, ldr, d, Y, ldy, mean, rstd, mask);
    else launch_forward<false, false>(nb, s, X, ldx, nrows, f, l2, gamma, beta, (float)eps, R, ldr, d, Y, ldy, mean, rstd, mask);
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
        double *rec = sums ? (double *)ws : nullptr;
#define PGCN_LN_BWD(V, C, S) launch_backward<V, C, S>(nb, s, G, ldg, X, ldx, nrows, (int)f, l2, mean, rstd, gamma, mask, scale, dX, lddx, rec)
        if (sums) {
            if (vec && cross) PGCN_LN_BWD(true, true, true);
            else if (vec) PGCN_LN_BWD(true, false, true);
            else if (cross) PGCN_LN_BWD(false, true, true);
            else PGCN_LN_BWD(false, false, true);
        } else {
            if (vec && cross) PGCN_LN_BWD(true, true, false);
            else if (vec) PGCN_LN_BWD(true, false, false);
            else if (cross) PGCN_LN_BWD(false, true, false);
            else PGCN_LN_BWD(false, false, false);
        }
#undef PGCN_LN_BWD
        PGCN_HIP_CHECK(hipGetLastError());
    }
    if (sums) {
        hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((2 * f + kFinalCols - 1) / kFinalCols)), dim3(kThreads), 0, s, (const double *)ws,
                           nb, (int)f, dbeta, dgamma);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    return PGCN_OK;
}
