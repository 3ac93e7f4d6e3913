// pgcn_gat_tail.hip -- the tail of a GAT layer in one pass each way, for gfx950 (PGAT.py: _GatTail; include/pgcn_hip.h has the
// contract): the heads of the aggregation's output X (nrows x heads * d, heads side by side) are kept or averaged, the bias joins,
// then ELU and the dropout keep function.
//
//   forward    r = mean ? (((X_0 + X_1) + X_2) + ...) (1 / heads) : X;   t = r + b;   a = elu ? (t > 0 ? t : expm1f(t)) : t;
//              Y = keep ? a s : 0                                                        pgcn_gat_tail_forward_f32   (one launch)
//   backward   deriv = (!elu || Y > 0) ? 1 : Y (1 / s) + 1;   Gm = keep ? (G s) deriv : 0;   dX_k = mean ? Gm (1 / heads) : Gm;
//              dbias = float(sum_i Gm)                                                   pgcn_gat_tail_backward_f32  (one pass + the
//                                                                                        second level of the column sums)
// ELU' = elu + 1 where the pre-activation is not positive, and elu = Y / s where the element was kept: the saved output gives the
// derivative.  It does NOT give the mask (Y == 0 is a dropped element or a == 0), and X is not kept for the backward, so the keep
// bits are formed again from the key: one fmix32 per element, no mask tensor written or read.
//
// The layout of pgcn_rowband.h over the OUTPUT columns (fout <= 1024), four rows per thread in flight; in mean mode a thread reads
// its four columns of every head (heads strided loads per output quad, so the float4 path needs d % 4 == 0) and adds them in index
// order.  The dropout pieces and the deterministic column sums (dbias: partial records [fout]) are those of pgcn_rowband.h too.
// This file is compiled with contraction off.  Raw pointers + a stream, no allocation, no synchronisation: graph-capturable.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"
#include "pgcn_rowband.h"

namespace {

constexpr int kMaxIn = 8192;       // widest input (heads * d); kMaxF bounds the output

__device__ __forceinline__ float elu(float t) { return t > 0.f ? t : expm1f(t); }      // (NaN stays NaN, -0.0 stays -0.0)

// `f` is the OUTPUT width (d in mean mode, heads * d otherwise); in mean mode head k of a row starts at column k * f of X.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void forward_kernel(const float *X, int64_t ldx, const float *__restrict__ bias, int64_t nrows, int f,
                                                           int nsum, float inv_heads, int log2_tpr, int act, DropArgs d, float *Y,
                                                           int64_t ldy) {
#pragma clang fp contract(off)
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kApplyRows, nrows);
    if (c0 >= f) return;
    const bool has_bias = bias != nullptr;
    float b[4] = {0.f, 0.f, 0.f, 0.f};
    if (has_bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = c0 + j < f ? bias[c0 + j] : 0.f;
    }
    const DropCols dc = drop_cols(d.step, d.seed, d.layer, c0);
    for (int64_t r = r0 + rg; r < rend; r += 4 * (int64_t)ngroups) {
        Quad p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr < rend) p[k] = load_quad<VEC>(X + rr * ldx, c0, f);
        }
        for (int h = 1; h < nsum; ++h) {                 // mean mode: the heads in index order, four rows' loads in flight
            Quad q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t rr = r + (int64_t)k * ngroups;
                if (rr < rend) q[k] = load_quad<VEC>(X + rr * ldx + (int64_t)h * f, c0, f);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (r + (int64_t)k * ngroups < rend) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) p[k].v[j] = p[k].v[j] + q[k].v[j];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr >= rend) break;
            Quad y;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float t = p[k].v[j];
                if (nsum > 1) t = t * inv_heads;
                if (has_bias) t = t + b[j];
                y.v[j] = act ? elu(t) : t;
            }
            if (dc.on) {
                const DropRow dr = drop_row(d.row_ids, dc, rr);
#pragma unroll
                for (int j = 0; j < 4; ++j) y.v[j] = drop_keep(dc, dr, j, d.thr) ? y.v[j] * d.scale : 0.f;
            }
            store_quad<VEC>(Y + rr * ldy, c0, f, y);
        }
    }
}

// One pass over G (and Y): writes dX (dX != NULL; in mean mode the same quad, scaled, to every head) and, when ws != NULL, the
// band's column sums of Gm in double.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void backward_kernel(const float *G, int64_t ldg, const float *__restrict__ Y, int64_t ldy,
                                                            int64_t nrows, int f, int nsum, float inv_heads, int log2_tpr, int act,
                                                            DropArgs d, float *dX, int64_t lddx, double *__restrict__ ws) {
#pragma clang fp contract(off)
    __shared__ double sm[4 * kThreads];
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kSumRows, nrows);
    const bool active = c0 < f;
    double acc[4] = {0, 0, 0, 0};
    if (active) {
        const DropCols dc = drop_cols(d.step, d.seed, d.layer, c0);
        const bool drop = dc.on;
        for (int64_t r = r0 + rg; r < rend; r += 4 * (int64_t)ngroups) {
            Quad g[4], y[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t rr = r + (int64_t)k * ngroups;
                if (rr < rend) {
                    g[k] = load_quad<VEC>(G + rr * ldg, c0, f);
                    if (act) y[k] = load_quad<VEC>(Y + rr * ldy, c0, f);
                    else y[k] = Quad{{0.f, 0.f, 0.f, 0.f}};
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t rr = r + (int64_t)k * ngroups;
                if (rr >= rend) break;
                const DropRow dr = drop ? drop_row(d.row_ids, dc, rr) : DropRow{0, 0};
                Quad o, x;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float gm = g[k].v[j];
                    if (drop) gm = gm * d.scale;
                    if (act && !(y[k].v[j] > 0.f)) {
                        float e = y[k].v[j];
                        if (drop) e = e * d.inv_scale;
                        gm = gm * (e + 1.0f);
                    }
                    if (drop && !drop_keep(dc, dr, j, d.thr)) gm = 0.f;
                    o.v[j] = gm;
                    acc[j] += (double)gm;                // (a lane beyond the last column loaded zeros: it adds zeros and stores nothing)
                    x.v[j] = nsum > 1 ? gm * inv_heads : gm;
                }
                if (dX) {
                    for (int h = 0; h < nsum; ++h) store_quad<VEC>(dX + rr * lddx + (int64_t)h * f, c0, f, x);
                }
            }
        }
    }
    if (ws == nullptr) return;                           // (uniform over the block: no barrier is skipped by a part of it)
    fold_row_groups(acc, sm, log2_tpr);
    if (rg == 0 && active) write_partial(acc, ws, blockIdx.x, c0, f);
}

// Second level of the f sums.  No record (nrows == 0): zeros.
__global__ __launch_bounds__(kThreads) void finalize_kernel(const double *__restrict__ ws, int64_t nbands, int f, float *__restrict__ dbias) {
    final_sum<1>(ws, nbands, f, [=](int o, double v) { dbias[o] = (float)v; });
}

}  // namespace

extern "C" int64_t pgcn_gat_tail_ws_bytes(int64_t nrows, int32_t fout) { return ws_bytes(nrows, fout, 1); }

extern "C" int pgcn_gat_tail_forward_f32(const float *X, int64_t ldx, int64_t nrows, int32_t heads, int32_t d, int32_t mean,
                                         const float *bias, int32_t act, const int64_t *row_ids, uint64_t seed, const int64_t *step,
                                         uint32_t layer, uint32_t thr, float *Y, int64_t ldy, pgcn_stream_t stream) {
    if (nrows < 0 || heads < 1 || d < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_forward_f32: nrows < 0, heads < 1 or d < 1");
    if (act != 0 && act != 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_forward_f32: act must be 0 (none) or 1 (ELU)");
    const int64_t fin = (int64_t)heads * d, fout = mean ? (int64_t)d : fin;
    if (ldx < fin || ldy < fout) return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_forward_f32: a leading dimension is below the width");
    if (nrows > 0 && (!X || !Y)) return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_forward_f32: null pointer");
    if (step && (uintptr_t)step % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_forward_f32: step must be 8-byte aligned");
    if (row_ids && (uintptr_t)row_ids % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_forward_f32: row_ids must be 8-byte aligned");
    if (Y && Y == X && (mean || ldy != ldx))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_forward_f32: in place (Y == X) needs mean == 0 and ldy == ldx");
    if (fout > kMaxF || fin > kMaxIn)
        return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_gat_tail_forward_f32: more than 1024 output or 8192 input columns");
    if (nrows == 0) return PGCN_OK;
    const DropArgs da = drop_args(row_ids, seed, step, layer, thr);
    const int f = (int)fout, nsum = mean ? (int)heads : 1;
    const float inv_heads = 1.0f / (float)heads;
    const bool vec = f % 4 == 0 && rows16(ldx) && rows16(ldy) && aligned16(X) && aligned16(Y);
    launch(vec ? forward_kernel<true> : forward_kernel<false>, apply_blocks(nrows), (hipStream_t)stream, X, ldx, bias, nrows, f, nsum,
           inv_heads, log2_threads_per_row(f), act, da, Y, ldy);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_gat_tail_backward_f32(const float *G, int64_t ldg, const float *Y, int64_t ldy, int64_t nrows, int32_t heads, int32_t d,
                                          int32_t mean, int32_t act, const int64_t *row_ids, uint64_t seed, const int64_t *step,
                                          uint32_t layer, uint32_t thr, float *dX, int64_t lddx, float *dbias, void *ws, int64_t ws_bytes,
                                          pgcn_stream_t stream) {
    if (nrows < 0 || heads < 1 || d < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_backward_f32: nrows < 0, heads < 1 or d < 1");
    if (act != 0 && act != 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_backward_f32: act must be 0 (none) or 1 (ELU)");
    const int64_t fin = (int64_t)heads * d, fout = mean ? (int64_t)d : fin;
    if (ldg < fout || (act && ldy < fout) || (dX && lddx < fin))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_backward_f32: a leading dimension is below the width");
    if (nrows > 0 && (!G || (act && !Y))) return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_backward_f32: null pointer");
    if (dbias && !ws) return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_backward_f32: dbias needs a work-space");
    if (dbias && (uintptr_t)ws % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_backward_f32: ws must be 8-byte aligned");
    if (step && (uintptr_t)step % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_backward_f32: step must be 8-byte aligned");
    if (row_ids && (uintptr_t)row_ids % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_backward_f32: row_ids must be 8-byte aligned");
    if (dX && dX == G && (mean || lddx != ldg))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_gat_tail_backward_f32: in place (dX == G) needs mean == 0 and lddx == ldg");
    if (fout > kMaxF || fin > kMaxIn)
        return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_gat_tail_backward_f32: more than 1024 output or 8192 input columns");
    if (dbias && ws_bytes < pgcn_gat_tail_ws_bytes(nrows, (int32_t)fout))
        return pgcn_set_error(PGCN_ENOMEM, "pgcn_gat_tail_backward_f32: work-space too small");
    if (!dbias && (!dX || nrows == 0)) return PGCN_OK;                    // nothing asked for
    const DropArgs da = drop_args(row_ids, seed, step, layer, thr);
    const int f = (int)fout, nsum = mean ? (int)heads : 1;
    const float inv_heads = 1.0f / (float)heads;
    const int64_t nb = bands(nrows);
    const int l2 = log2_threads_per_row(f);
    hipStream_t s = (hipStream_t)stream;
    if (nb > 0) {
        const bool vec = f % 4 == 0 && rows16(ldg) && aligned16(G) && (!act || (rows16(ldy) && aligned16(Y))) &&
                         (!dX || (rows16(lddx) && aligned16(dX)));
        double *rec = dbias ? (double *)ws : nullptr;
        launch(vec ? backward_kernel<true> : backward_kernel<false>, nb, s, G, ldg, Y, ldy, nrows, f, nsum, inv_heads, l2, act, da, dX, lddx,
               rec);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    if (dbias) {
        launch(finalize_kernel, final_blocks(f), s, ws, nb, f, dbias);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    return PGCN_OK;
}
