// pgcn_gat_tail_ln.hip -- the tail of a GAT layer WITH a per-vertex layer norm and a residual link, one pass each way, for gfx950
// (PGAT.py: _GatTailNorm; include/pgcn_hip.h has the contract).  The order is the GCN layers': convolution, norm, activation,
// dropout, plus the input.
//
//   forward    r = mean ? (((X_0 + X_1) + X_2) + ...) (1 / heads) : X;   t = r + b            (pgcn_gat_tail.hip's arithmetic)
//              mean_i = sum_j t / fout;  var_i = sum_j (t - mean_i)^2 / fout;  rstd_i = 1 / sqrt(var_i + eps)   (two passes, in registers)
//              xh = (t - mean_i) rstd_i;  u = fma(gamma_j, xh, beta_j);  a = elu ? (u > 0 ? u : expm1f(u)) : u
//              dd = keep ? a s : 0;  Y = R ? R + dd : dd                              pgcn_gat_tail_ln_forward_f32   (one launch)
//   backward   t, xh, u again from X;  deriv = (elu && u <= 0) ? expf(u) : 1;  g' = keep ? (G s) deriv : 0;  gh = g' gamma_j
//              c1 = sum_j gh / fout;  c2 = sum_j gh xh / fout;  dT = rstd_i ((gh - c1) - xh c2);  dX_k = mean ? dT (1 / heads) : dT
//              dbias_j = float(sum_i dT);  dgamma_j = float(sum_i g' xh);  dbeta_j = float(sum_i g')
//                                                                                     pgcn_gat_tail_ln_backward_f32  (one pass + the
//                                                                                     second level of the column sums)
// Nothing of size nrows x fout lives from the forward to the backward: the engine keeps X for its own backward, the sign of u comes
// from forming u again, the keep bits from the key; 2 nrows floats (mean, rstd) are saved.  pgcn_layernorm.hip keeps a bit per
// element instead: its X is a dense product's output that nothing else holds on to, so it has to be saved either way, and the bits
// spare the hash and the fma; here X is alive already and the recompute costs no pass and no spill (DESIGN.md 4 has the registers).
//
// The layout of pgcn_rowband.h over the OUTPUT columns, two rows per thread in flight; in mean mode a thread reads its four columns
// of every head and adds them in index order before the first row reduction.  Row sums (fp32): a thread adds its quad
// ((q0 + q1) + q2) + q3, columns at and beyond fout as zeros; then an xor butterfly over the row's aligned group of TPR lanes
// (TPR <= 64: inside one wave); TPR = 128 or 256: the butterfly over the whole wave, lane 0 of each wave leaves its partial in LDS,
// every thread adds its row's 2 or 4 partials as (p0 + p1) [+ (p2 + p3)] -- the tree of pgcn_layernorm.hip.  Nothing in it knows the
// row's index, the block or nrows: a row's results are a function of the row.  EVERY thread of a block walks every iteration (rows
// beyond the band and columns beyond fout compute on zeros and store nothing): the shuffles and the barriers are never divergent.
//
// Column sums of the backward (partial records [3][fout]: dT, g' xh, g') and the dropout pieces: those of pgcn_rowband.h.  A
// dropped element adds exact zeros to dgamma and dbeta whatever its x.  csrc/build.sh compiles this file with -ffp-contract=off:
// the one fused operation is the written fmaf.  Raw pointers + a stream, no allocation, no synchronisation: graph-capturable.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"
#include "pgcn_rowband.h"

namespace {

constexpr int kMaxIn = 8192;       // widest input (heads * d); kMaxF bounds the output
constexpr int kWaves = kThreads / 64;
constexpr int kInFlight = 2;       // rows a thread holds at once
constexpr int kRec = 3;            // sums of a record: dbias, dgamma, dbeta

__device__ __forceinline__ float quad_sum(const float (&e)[4]) { return ((e[0] + e[1]) + e[2]) + e[3]; }

// v[k] <- the sum of v[k] over the tpr threads of this thread's row, k < NV, the same bits in every one of them.  CROSS (tpr = 128 or
// 256): `sm` holds 2 x NV x kWaves floats, `phase` picks the half -- successive calls alternate, so that ONE barrier per call is
// enough (a wave that runs ahead writes the other half; the half it will write after that was last read before the barrier between).
template <int NV, bool CROSS>
__device__ __forceinline__ void row_sums(float (&v)[NV], int tpr, float *sm, int phase, int tid) {
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

// What both directions need of the heads: t of kInFlight rows.  `f` is the OUTPUT width; in mean mode head h of a row starts at
// column h * f of X.  A row that is not `ok` and a column at or beyond f give t = 0 (the bias of such a column was loaded as 0).
struct Heads {
    int nsum;
    float inv_heads;
    bool has_bias;
};

template <bool VEC>
__device__ __forceinline__ void load_t(const float *X, int64_t ldx, const int64_t (&rr)[kInFlight], const bool (&ok)[kInFlight], int c0,
                                       int f, const Heads &hd, const Quad &b, Quad (&t)[kInFlight]) {
#pragma unroll
    for (int k = 0; k < kInFlight; ++k) {
        if (ok[k]) t[k] = load_quad<VEC>(X + rr[k] * ldx, c0, f);
        else t[k] = Quad{{0.f, 0.f, 0.f, 0.f}};
    }
    for (int h = 1; h < hd.nsum; ++h) {                  // mean mode: the heads in index order, both rows' loads in flight
        Quad q[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            if (ok[k]) q[k] = load_quad<VEC>(X + rr[k] * ldx + (int64_t)h * f, c0, f);
            else q[k] = Quad{{0.f, 0.f, 0.f, 0.f}};
        }
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) t[k].v[j] = t[k].v[j] + q[k].v[j];
        }
    }
#pragma unroll
    for (int k = 0; k < kInFlight; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = t[k].v[j];
            if (hd.nsum > 1) v = v * hd.inv_heads;
            if (hd.has_bias && ok[k]) v = v + b.v[j];
            t[k].v[j] = v;
        }
    }
}

template <bool VEC, bool CROSS>
__global__ __launch_bounds__(kThreads) void forward_kernel(const float *X, int64_t ldx, const float *__restrict__ bias, int64_t nrows, int f,
                                                           int nsum, float inv_heads, int log2_tpr, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, float eps, int act, const float *R, int64_t ldr,
                                                           DropArgs d, float *Y, int64_t ldy, float *__restrict__ mean,
                                                           float *__restrict__ rstd) {
    __shared__ float sm[2 * kInFlight * kWaves];
    const int tid = threadIdx.x;
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kApplyRows, nrows);
    const bool active = c0 < f;
    const float ff = (float)f;
    const Heads hd = {nsum, inv_heads, bias != nullptr};
    const Quad b = hd.has_bias ? load_cols(bias, c0, f) : Quad{{0.f, 0.f, 0.f, 0.f}};
    const Quad ga = load_cols(gamma, c0, f), be = load_cols(beta, c0, f);
    const DropCols dc = drop_cols(d.step, d.seed, d.layer, c0);
    for (int64_t base = r0; base < rend; base += kInFlight * (int64_t)ngroups) {          // (uniform over the block)
        int64_t rr[kInFlight];
        bool ok[kInFlight];
        Quad t[kInFlight];
        float s[kInFlight], mu[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            rr[k] = base + (int64_t)k * ngroups + rg;
            ok[k] = rr[k] < rend && active;
        }
        load_t<VEC>(X, ldx, rr, ok, c0, f, hd, b, t);
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) s[k] = quad_sum(t[k].v);
        row_sums<kInFlight, CROSS>(s, tpr, sm, 0, tid);
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            mu[k] = s[k] / ff;
            float e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float c = t[k].v[j] - mu[k];
                e[j] = c0 + j < f ? c * c : 0.f;
            }
            s[k] = quad_sum(e);
        }
        row_sums<kInFlight, CROSS>(s, tpr, sm, 1, tid);
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            if (!ok[k]) continue;
            const float rs = 1.0f / sqrtf(s[k] / ff + eps);
            const DropRow dr = dc.on ? drop_row(d.row_ids, dc, rr[k]) : DropRow{0, 0};
            Quad y;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = (t[k].v[j] - mu[k]) * rs;
                const float uu = fmaf(ga.v[j], xh, be.v[j]);
                float v = act ? (uu > 0.f ? uu : expm1f(uu)) : uu;                        // (NaN stays NaN)
                if (dc.on) v = drop_keep(dc, dr, j, d.thr) ? v * d.scale : 0.f;
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
                rstd[rr[k]] = rs;
            }
        }
    }
}

// One pass over G and X: writes dX (dX != NULL; in mean mode the same quad, scaled, to every head) and, with SUMS, the band's record.
template <bool VEC, bool CROSS, bool SUMS>
__global__ __launch_bounds__(kThreads) void backward_kernel(const float *G, int64_t ldg, const float *X, int64_t ldx,
                                                            const float *__restrict__ bias, int64_t nrows, int f, int nsum, float inv_heads,
                                                            int log2_tpr, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            const float *__restrict__ mean, const float *__restrict__ rstd, int act,
                                                            DropArgs d, float *dX, int64_t lddx, double *__restrict__ ws) {
    __shared__ float sm[2 * 2 * kInFlight * kWaves];
    __shared__ double smd[SUMS ? 4 * kRec * kThreads : 1];
    const int tid = threadIdx.x;
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kSumRows, nrows);
    const bool active = c0 < f;
    const float ff = (float)f;
    const Heads hd = {nsum, inv_heads, bias != nullptr};
    const Quad b = hd.has_bias ? load_cols(bias, c0, f) : Quad{{0.f, 0.f, 0.f, 0.f}};
    const Quad ga = load_cols(gamma, c0, f), be = load_cols(beta, c0, f);
    const DropCols dc = drop_cols(d.step, d.seed, d.layer, c0);
    double acc[4 * kRec] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int phase = 0;
    for (int64_t base = r0; base < rend; base += kInFlight * (int64_t)ngroups, ++phase) {  // (uniform over the block)
        int64_t rr[kInFlight];
        bool ok[kInFlight];
        Quad t[kInFlight], g[kInFlight], gh[kInFlight];
        float rs[kInFlight], s[2 * kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            rr[k] = base + (int64_t)k * ngroups + rg;
            ok[k] = rr[k] < rend && active;
            if (ok[k]) g[k] = load_quad<VEC>(G + rr[k] * ldg, c0, f);
            else g[k] = Quad{{0.f, 0.f, 0.f, 0.f}};
        }
        load_t<VEC>(X, ldx, rr, ok, c0, f, hd, b, t);
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            float mu = 0.f;
            rs[k] = 0.f;
            DropRow dr = {0, 0};
            if (ok[k]) {
                mu = mean[rr[k]];
                rs[k] = rstd[rr[k]];
                if (dc.on) dr = drop_row(d.row_ids, dc, rr[k]);
            }
            float p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = (t[k].v[j] - mu) * rs[k];                                // (t now holds xh)
                const float uu = fmaf(ga.v[j], xh, be.v[j]);
                const bool keep = ok[k] && c0 + j < f && (!dc.on || drop_keep(dc, dr, j, d.thr));
                float gm = g[k].v[j];
                if (dc.on) gm = gm * d.scale;
                if (act && uu <= 0.f) gm = gm * expf(uu);
                if (!keep) gm = 0.f;
                t[k].v[j] = xh;
                gh[k].v[j] = gm * ga.v[j];
                p[j] = gh[k].v[j] * xh;
                if constexpr (SUMS) {
                    // a dropped element adds exact zeros whatever its x: a NaN or inf there must not reach the column's sums
                    acc[4 + j] += keep ? (double)gm * (double)xh : 0.0;
                    acc[8 + j] += (double)gm;
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
                const float w = t[k].v[j] * c2;
                const float dt = rs[k] * ((gh[k].v[j] - c1) - w);
                if constexpr (SUMS) {
                    if (c0 + j < f) acc[j] += (double)dt;
                }
                o.v[j] = nsum > 1 ? dt * inv_heads : dt;
            }
            if (dX) {
                for (int h = 0; h < nsum; ++h) store_quad<VEC>(dX + rr[k] * lddx + (int64_t)h * f, c0, f, o);
            }
        }
    }
    if constexpr (SUMS) {
        fold_row_groups(acc, smd, log2_tpr);
        if (rg == 0 && active) {
            double *rec = ws + (int64_t)blockIdx.x * kRec * f;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c0 + j < f) {
#pragma unroll
                    for (int q = 0; q < kRec; ++q) rec[q * f + c0 + j] = acc[4 * q + j];
                }
        }
    }
}

// Second level of the 3 f sums: dbias, dgamma, dbeta in that order.  No record (nrows == 0): zeros.
__global__ __launch_bounds__(kThreads) void finalize_kernel(const double *__restrict__ ws, int64_t nbands, int f, float *__restrict__ dbias,
                                                            float *__restrict__ dgamma, float *__restrict__ dbeta) {
    final_sum<kRec>(ws, nbands, f, [=](int o, double v) {
        if (o < f) dbias[o] = (float)v;
        else if (o < 2 * f) dgamma[o - f] = (float)v;
        else dbeta[o - 2 * f] = (float)v;
    });
}

bool eps_ok(double eps) { return eps > 0.0 && eps <= DBL_MAX && (float)eps > 0.f && (float)eps <= FLT_MAX; }

// picks the <VEC, CROSS> instance of a kernel template with two or three bool parameters
#define PGCN_PICK2(K, vec, cross) \
    ((cross) ? ((vec) ? K<true, true> : K<false, true>) : ((vec) ? K<true, false> : K<false, false>))
#define PGCN_PICK3(K, vec, cross, S) \
    ((cross) ? ((vec) ? K<true, true, S> : K<false, true, S>) : ((vec) ? K<true, false, S> : K<false, false, S>))

}  // namespace

extern "C" int64_t pgcn_gat_tail_ln_ws_bytes(int64_t nrows, int32_t fout) { return ws_bytes(nrows, fout, kRec); }

extern "C" int pgcn_gat_tail_ln_forward_f32(const float *X, int64_t ldx, int64_t nrows, int32_t heads, int32_t d, int32_t mean_heads,
                                            const float *bias, const float *gamma, const float *beta, double eps, int32_t act,
                                            const float *R, int64_t ldr, const int64_t *row_ids, uint64_t seed, const int64_t *step,
                                            uint32_t layer, uint32_t thr, float *Y, int64_t ldy, float *mean, float *rstd,
                                            pgcn_stream_t stream) {
#define WHO "pgcn_gat_tail_ln_forward_f32: "
    if (nrows < 0 || heads < 1 || d < 1) return pgcn_set_error(PGCN_EINVAL, WHO "nrows < 0, heads < 1 or d < 1");
    if (act != 0 && act != 1) return pgcn_set_error(PGCN_EINVAL, WHO "act must be 0 (none) or 1 (ELU)");
    const int64_t fin = (int64_t)heads * d, fout = mean_heads ? (int64_t)d : fin;
    if (ldx < fin || ldy < fout || (R && ldr < fout)) return pgcn_set_error(PGCN_EINVAL, WHO "a leading dimension is below the width");
    if (!gamma || !beta || (nrows > 0 && (!X || !Y))) return pgcn_set_error(PGCN_EINVAL, WHO "null pointer");
    if (!eps_ok(eps)) return pgcn_set_error(PGCN_EINVAL, WHO "eps must be finite and > 0");
    if (step && (uintptr_t)step % 8 != 0) return pgcn_set_error(PGCN_EINVAL, WHO "step must be 8-byte aligned");
    if (row_ids && (uintptr_t)row_ids % 8 != 0) return pgcn_set_error(PGCN_EINVAL, WHO "row_ids must be 8-byte aligned");
    if ((mean != nullptr) != (rstd != nullptr)) return pgcn_set_error(PGCN_EINVAL, WHO "mean and rstd go together (both or neither)");
    if (Y && Y == R && ldy != ldr) return pgcn_set_error(PGCN_EINVAL, WHO "in place (Y == R) needs ldy == ldr");
    if (Y && Y == X) return pgcn_set_error(PGCN_EINVAL, WHO "Y must not be X (the backward reads X)");
    if (fout > kMaxF || fin > kMaxIn) return pgcn_set_error(PGCN_EUNSUPPORTED, WHO "more than 1024 output or 8192 input columns");
    if (nrows == 0) return PGCN_OK;
    const int f = (int)fout, l2 = log2_threads_per_row(f);
    const bool vec = f % 4 == 0 && rows16(ldx) && rows16(ldy) && aligned16(X) && aligned16(Y) && (!R || (rows16(ldr) && aligned16(R)));
    launch(PGCN_PICK2(forward_kernel, vec, l2 > 6), apply_blocks(nrows), (hipStream_t)stream, X, ldx, bias, nrows, f,
           mean_heads ? (int)heads : 1, 1.0f / (float)heads, l2, gamma, beta, (float)eps, act, R, ldr,
           drop_args(row_ids, seed, step, layer, thr), Y, ldy, mean, rstd);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_gat_tail_ln_backward_f32(const float *G, int64_t ldg, const float *X, int64_t ldx, int64_t nrows, int32_t heads,
                                             int32_t d, int32_t mean_heads, const float *bias, const float *gamma, const float *beta,
                                             const float *mean, const float *rstd, int32_t act, const int64_t *row_ids, uint64_t seed,
                                             const int64_t *step, uint32_t layer, uint32_t thr, float *dX, int64_t lddx, float *dbias,
                                             float *dgamma, float *dbeta, void *ws, int64_t ws_bytes, pgcn_stream_t stream) {
#undef WHO
#define WHO "pgcn_gat_tail_ln_backward_f32: "
    if (nrows < 0 || heads < 1 || d < 1) return pgcn_set_error(PGCN_EINVAL, WHO "nrows < 0, heads < 1 or d < 1");
    if (act != 0 && act != 1) return pgcn_set_error(PGCN_EINVAL, WHO "act must be 0 (none) or 1 (ELU)");
    const int64_t fin = (int64_t)heads * d, fout = mean_heads ? (int64_t)d : fin;
    if (ldg < fout || ldx < fin || (dX && lddx < fin)) return pgcn_set_error(PGCN_EINVAL, WHO "a leading dimension is below the width");
    if (!gamma || !beta || (nrows > 0 && (!G || !X || !mean || !rstd))) return pgcn_set_error(PGCN_EINVAL, WHO "null pointer");
    if ((dbias != nullptr) != (dgamma != nullptr) || (dbias != nullptr) != (dbeta != nullptr))
        return pgcn_set_error(PGCN_EINVAL, WHO "dbias, dgamma and dbeta go together (all three or none)");
    const bool sums = dbias != nullptr;
    if (sums && !ws) return pgcn_set_error(PGCN_EINVAL, WHO "the sums need a work-space");
    if (sums && (uintptr_t)ws % 8 != 0) return pgcn_set_error(PGCN_EINVAL, WHO "ws must be 8-byte aligned");
    if (step && (uintptr_t)step % 8 != 0) return pgcn_set_error(PGCN_EINVAL, WHO "step must be 8-byte aligned");
    if (row_ids && (uintptr_t)row_ids % 8 != 0) return pgcn_set_error(PGCN_EINVAL, WHO "row_ids must be 8-byte aligned");
    if (dX && (dX == G || dX == X) && (mean_heads || lddx != (dX == G ? ldg : ldx)))
        return pgcn_set_error(PGCN_EINVAL, WHO "in place (dX == G or dX == X) needs mean == 0 and equal leading dimensions");
    if (fout > kMaxF || fin > kMaxIn) return pgcn_set_error(PGCN_EUNSUPPORTED, WHO "more than 1024 output or 8192 input columns");
    if (sums && ws_bytes < pgcn_gat_tail_ln_ws_bytes(nrows, (int32_t)fout)) return pgcn_set_error(PGCN_ENOMEM, WHO "work-space too small");
    if (!sums && (!dX || nrows == 0)) return PGCN_OK;                     // nothing asked for
    const int f = (int)fout, l2 = log2_threads_per_row(f);
    const int64_t nb = bands(nrows);
    hipStream_t s = (hipStream_t)stream;
    if (nb > 0) {
        const bool vec = f % 4 == 0 && rows16(ldg) && rows16(ldx) && aligned16(G) && aligned16(X) && (!dX || (rows16(lddx) && aligned16(dX)));
        const bool cross = l2 > 6;
        launch(sums ? PGCN_PICK3(backward_kernel, vec, cross, true) : PGCN_PICK3(backward_kernel, vec, cross, false), nb, s, G, ldg, X, ldx,
               bias, nrows, f, mean_heads ? (int)heads : 1, 1.0f / (float)heads, l2, gamma, beta, mean, rstd, act,
               drop_args(row_ids, seed, step, layer, thr), dX, lddx, sums ? (double *)ws : nullptr);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    if (sums) {
        launch(finalize_kernel, final_blocks(kRec * f), s, (const double *)ws, nb, f, dbias, dgamma, dbeta);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    return PGCN_OK;
}
