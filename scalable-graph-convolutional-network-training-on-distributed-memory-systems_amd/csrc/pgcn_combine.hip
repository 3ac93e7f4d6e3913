// pgcn_combine.hip -- the tail of a GraphSAGE-style layer in one pass each way, for gfx950 (PGCN.py: _CombineBiasReluDropout;
// include/pgcn_hip.h has the contract): the neighbour product Z1 = (A H) W_n^T and the root product Z2 = H W_r^T are added, the
// bias joins, then the ReLU and the dropout keep function.
//
//   forward    t = (Z1 + Z2) + b;   Y = relu ? (keep ? max(0, t) s : 0) : t        pgcn_combine_forward_f32   (one launch)
//   backward   Gm = relu ? (Y > 0 ? G s : 0) : G;   dbias = float(sum_i Gm)         pgcn_combine_backward_f32  (one pass + the
//                                                                                   second level of the column sums)
// The saved output is its own mask (Y > 0 exactly where the element was kept and its pre-activation positive); Gm is the operand
// of BOTH products' backward: one write, read by four GEMMs.  Neither Z is needed by the backward, so Y may be written over Z1.
//
// The layout of the kernels, the dropout pieces and the deterministic column sums (dbias: partial records [f]) are those of
// pgcn_rowband.h; contraction is off in every body.  Raw pointers + a stream, no allocation, no synchronisation: graph-capturable.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"
#include "pgcn_rowband.h"

namespace {

// The elements' arithmetic, each operation rounded to fp32 on its own.  An absent term is not added at all (a -0.0 survives).
__device__ __forceinline__ float combine(float z1, float z2, float b, bool has_z2, bool has_bias) {
#pragma clang fp contract(off)
    float t = z1;
    if (has_z2) t = t + z2;
    if (has_bias) t = t + b;
    return t;
}
__device__ __forceinline__ float relu(float t) { return t < 0.f ? 0.f : t; }      // (NaN stays NaN)
__device__ __forceinline__ float masked_grad(float g, float y, float scale) {
#pragma clang fp contract(off)
    return y > 0.f ? g * scale : 0.f;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void forward_kernel(const float *Z1, int64_t ldz1, const float *Z2, int64_t ldz2,
                                                           const float *__restrict__ bias, int64_t nrows, int f, int log2_tpr, int do_relu,
                                                           DropArgs d, float *Y, int64_t ldy) {
#pragma clang fp contract(off)
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kApplyRows, nrows);
    if (c0 >= f) return;
    const bool has_z2 = Z2 != nullptr, has_bias = bias != nullptr;
    float b[4] = {0.f, 0.f, 0.f, 0.f};
    if (has_bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = c0 + j < f ? bias[c0 + j] : 0.f;
    }
    const DropCols dc = drop_cols(d.step, d.seed, d.layer, c0, do_relu);
    for (int64_t r = r0 + rg; r < rend; r += 4 * (int64_t)ngroups) {
        Quad p[4], q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr < rend) {
                p[k] = load_quad<VEC>(Z1 + rr * ldz1, c0, f);
                if (has_z2) q[k] = load_quad<VEC>(Z2 + rr * ldz2, c0, f);
                else q[k] = Quad{{0.f, 0.f, 0.f, 0.f}};
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr >= rend) break;
            Quad y;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float t = combine(p[k].v[j], q[k].v[j], b[j], has_z2, has_bias);
                y.v[j] = do_relu ? relu(t) : t;
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

// One pass over G (and Y): writes Gm (Gm != NULL) and, when ws != NULL, the band's column sums of Gm in double.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void backward_kernel(const float *G, int64_t ldg, const float *__restrict__ Y, int64_t ldy,
                                                            int64_t nrows, int f, int log2_tpr, int do_relu, float scale, float *Gm,
                                                            int64_t ldgm, double *__restrict__ ws) {
#pragma clang fp contract(off)
    __shared__ double sm[4 * kThreads];
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kSumRows, nrows);
    const bool active = c0 < f;
    double acc[4] = {0, 0, 0, 0};
    if (active) {
        for (int64_t r = r0 + rg; r < rend; r += 4 * (int64_t)ngroups) {
            Quad g[4], y[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t rr = r + (int64_t)k * ngroups;
                if (rr < rend) {
                    g[k] = load_quad<VEC>(G + rr * ldg, c0, f);
                    if (do_relu) y[k] = load_quad<VEC>(Y + rr * ldy, c0, f);
                    else y[k] = Quad{{0.f, 0.f, 0.f, 0.f}};
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t rr = r + (int64_t)k * ngroups;
                if (rr >= rend) break;
                Quad o;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    o.v[j] = do_relu ? masked_grad(g[k].v[j], y[k].v[j], scale) : g[k].v[j];
                    acc[j] += (double)o.v[j];            // (a lane beyond the last column loaded zeros: it adds zeros and stores nothing)
                }
                if (Gm) store_quad<VEC>(Gm + rr * ldgm, c0, f, o);
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

extern "C" int64_t pgcn_combine_ws_bytes(int64_t nrows, int32_t f) { return ws_bytes(nrows, f, 1); }

extern "C" int pgcn_combine_forward_f32(const float *Z1, int64_t ldz1, const float *Z2, int64_t ldz2, const float *bias, int64_t nrows,
                                        int32_t f, int32_t relu, const int64_t *row_ids, uint64_t seed, const int64_t *step, uint32_t layer,
                                        uint32_t thr, float *Y, int64_t ldy, pgcn_stream_t stream) {
    if (nrows < 0 || f < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_combine_forward_f32: nrows < 0 or f < 1");
    if (ldz1 < f || ldy < f || (Z2 && ldz2 < f)) return pgcn_set_error(PGCN_EINVAL, "pgcn_combine_forward_f32: a leading dimension is below f");
    if (nrows > 0 && (!Z1 || !Y)) return pgcn_set_error(PGCN_EINVAL, "pgcn_combine_forward_f32: null pointer");
    if (step && (uintptr_t)step % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_combine_forward_f32: step must be 8-byte aligned");
    if (row_ids && (uintptr_t)row_ids % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_combine_forward_f32: row_ids must be 8-byte aligned");
    if (Y && Y == Z1 && ldy != ldz1)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_combine_forward_f32: in place (Y == Z1) needs ldy == ldz1");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_combine_forward_f32: more than 1024 columns");
    if (nrows == 0) return PGCN_OK;
    const bool vec = f % 4 == 0 && rows16(ldz1) && rows16(ldy) && aligned16(Z1) && aligned16(Y) && (!Z2 || (rows16(ldz2) && aligned16(Z2)));
    launch(vec ? forward_kernel<true> : forward_kernel<false>, apply_blocks(nrows), (hipStream_t)stream, Z1, ldz1, Z2, ldz2, bias, nrows, f,
           log2_threads_per_row(f), relu != 0, drop_args(row_ids, seed, relu ? step : nullptr, layer, thr), Y, ldy);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_combine_backward_f32(const float *G, int64_t ldg, const float *Y, int64_t ldy, int64_t nrows, int32_t f, int32_t relu,
                                         float scale, float *Gm, int64_t ldgm, float *dbias, void *ws, int64_t ws_bytes,
                                         pgcn_stream_t stream) {
    if (nrows < 0 || f < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_combine_backward_f32: nrows < 0 or f < 1");
    if (ldg < f || (relu && ldy < f) || (Gm && ldgm < f))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_combine_backward_f32: a leading dimension is below f");
    if (nrows > 0 && (!G || (relu && !Y))) return pgcn_set_error(PGCN_EINVAL, "pgcn_combine_backward_f32: null pointer");
    if (dbias && !ws) return pgcn_set_error(PGCN_EINVAL, "pgcn_combine_backward_f32: dbias needs a work-space");
    if (dbias && (uintptr_t)ws % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_combine_backward_f32: ws must be 8-byte aligned");
    if (!(scale > 0.f && scale <= FLT_MAX)) return pgcn_set_error(PGCN_EINVAL, "pgcn_combine_backward_f32: scale must be finite and > 0");
    if (Gm && Gm == G && ldgm != ldg)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_combine_backward_f32: in place (Gm == G) needs ldgm == ldg");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_combine_backward_f32: more than 1024 columns");
    if (dbias && ws_bytes < pgcn_combine_ws_bytes(nrows, f))
        return pgcn_set_error(PGCN_ENOMEM, "pgcn_combine_backward_f32: work-space too small");
    if (!dbias && (!Gm || nrows == 0)) return PGCN_OK;                    // nothing asked for
    const int64_t nb = bands(nrows);
    const int l2 = log2_threads_per_row(f);
    hipStream_t s = (hipStream_t)stream;
    if (nb > 0) {
        const bool vec = f % 4 == 0 && rows16(ldg) && aligned16(G) && (!relu || (rows16(ldy) && aligned16(Y))) &&
                         (!Gm || (rows16(ldgm) && aligned16(Gm)));
        double *rec = dbias ? (double *)ws : nullptr;
        launch(vec ? backward_kernel<true> : backward_kernel<false>, nb, s, G, ldg, Y, ldy, nrows, f, l2, relu != 0, scale, Gm, ldgm, rec);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    if (dbias) {
        launch(finalize_kernel, final_blocks(f), s, ws, nb, f, dbias);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    return PGCN_OK;
}
