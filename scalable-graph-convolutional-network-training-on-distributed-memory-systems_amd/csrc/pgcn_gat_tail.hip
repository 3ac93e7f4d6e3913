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
// Layout as in pgcn_combine.hip: 256 threads; a thread owns FOUR consecutive OUTPUT columns, TPR = the power of two >=
// ceil(fout / 4) threads span a row, 256 / TPR row groups walk a band of consecutive rows, four rows per thread in flight; in mean
// mode a thread reads its four columns of every head (heads strided loads per output quad) and adds them in index order.  The
// bias and the column's share of the dropout hash are loaded / formed once per thread, before the row loop.  fout <= 1024.  One
// float4 per thread, row and head when fout % 4 == 0 (so d % 4 == 0 in mean mode) and every base and leading dimension keeps the
// rows 16-byte aligned, four guarded scalars otherwise: the same thread does the same arithmetic in the same order, so both paths
// leave the same bits (this file is compiled with contraction off).
//
// dbias: as in pgcn_combine.hip -- a block of the backward owns kSumRows consecutive rows, adds Gm in double registers, folds the
// row groups through LDS by a fixed tree and writes ONE partial record [fout] of doubles; the second launch adds the records in a
// fixed order.  No floating-point atomics; a NaN or inf stays in its own column.  Raw pointers + a stream, no allocation, no
// synchronisation: graph-capturable.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"

#define PG_DROPOUT_FN __host__ __device__ __forceinline__
#include "../gemm/pgcn_dropout.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSumRows = 512;      // rows of a block of the backward (kernels.GAT_TAIL_SUM_ROWS restates it)
constexpr int kApplyRows = 128;    // rows of a block of the forward
constexpr int kFinalCols = 32;     // columns of a block of the second level
constexpr int kFinalGroups = kThreads / kFinalCols;
constexpr int kMaxF = 1024;        // widest output
constexpr int kMaxIn = 8192;       // widest input (heads * d)

struct Quad {
    float v[4];
};

// (no __restrict__ on the matrices: Y may be X itself; a thread reads its own elements before it writes them)
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

__device__ __forceinline__ float elu(float t) { return t > 0.f ? t : expm1f(t); }      // (NaN stays NaN, -0.0 stays -0.0)

struct DropArgs {
    const int64_t *row_ids;
    const int64_t *step;       // NULL: no dropout
    uint64_t seed;
    uint32_t layer, thr;
    float scale, inv_scale;
};

// `f` is the OUTPUT width (d in mean mode, heads * d otherwise); in mean mode head k of a row starts at column k * f of X.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void forward_kernel(const float *X, int64_t ldx, const float *__restrict__ bias, int64_t nrows, int f,
                                                           int nsum, float inv_heads, int log2_tpr, int act, DropArgs d, float *Y,
                                                           int64_t ldy) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, u = tid & ((1 << log2_tpr) - 1), rg = tid >> log2_tpr, ngroups = kThreads >> log2_tpr;
    const int c0 = 4 * u;
    if (c0 >= f) return;
    const int64_t r0 = (int64_t)blockIdx.x * kApplyRows;
    const int64_t rend = r0 + kApplyRows < nrows ? r0 + kApplyRows : nrows;
    const bool has_bias = bias != nullptr;
    float b[4] = {0.f, 0.f, 0.f, 0.f};
    if (has_bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = c0 + j < f ? bias[c0 + j] : 0.f;
    }
    const bool drop = d.step != nullptr;
    uint64_t key = 0;
    uint32_t dcol[4] = {0, 0, 0, 0};
    if (drop) {
        key = dropout_key(d.seed, (uint64_t)d.step[0], d.layer);
#pragma unroll
        for (int j = 0; j < 4; ++j) dcol[j] = dropout_col(key, (uint32_t)(c0 + j));      // the column's share: once per column
    }
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

// One pass over G (and Y): writes dX (dX != NULL; in mean mode the same quad, scaled, to every head) and, when ws != NULL, the
// band's column sums of Gm in double.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void backward_kernel(const float *G, int64_t ldg, const float *__restrict__ Y, int64_t ldy,
                                                            int64_t nrows, int f, int nsum, float inv_heads, int log2_tpr, int act,
                                                            DropArgs d, float *dX, int64_t lddx, double *__restrict__ ws) {
#pragma clang fp contract(off)
    __shared__ double sm[4 * kThreads];
    const int tid = threadIdx.x, u = tid & ((1 << log2_tpr) - 1), rg = tid >> log2_tpr, ngroups = kThreads >> log2_tpr;
    const int c0 = 4 * u;
    const bool active = c0 < f;
    const int64_t r0 = (int64_t)blockIdx.x * kSumRows;
    const int64_t rend = r0 + kSumRows < nrows ? r0 + kSumRows : nrows;
    double acc[4] = {0, 0, 0, 0};
    if (active) {
        const bool drop = d.step != nullptr;
        uint64_t key = 0;
        uint32_t dcol[4] = {0, 0, 0, 0};
        if (drop) {
            key = dropout_key(d.seed, (uint64_t)d.step[0], d.layer);
#pragma unroll
            for (int j = 0; j < 4; ++j) dcol[j] = dropout_col(key, (uint32_t)(c0 + j));
        }
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
                uint32_t term = 0, hi = 0;
                if (drop) {
                    const uint64_t grow = d.row_ids ? (uint64_t)d.row_ids[rr] : (uint64_t)rr;
                    term = dropout_row(key, grow), hi = (uint32_t)(grow >> 32);
                }
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
                    if (drop && dropout_u(dcol[j], term, hi) < d.thr) gm = 0.f;
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
    // fold the 256 / TPR row groups through LDS by a fixed tree, k-major: neighbouring threads touch neighbouring doubles
#pragma unroll
    for (int k = 0; k < 4; ++k) sm[k * kThreads + tid] = acc[k];
    for (int s = ngroups >> 1; s >= 1; s >>= 1) {
        __syncthreads();
        if (rg < s) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sm[k * kThreads + tid] += sm[k * kThreads + tid + (s << log2_tpr)];
        }
    }
    __syncthreads();
    if (rg == 0 && active) {
        double *rec = ws + (int64_t)blockIdx.x * f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < f) rec[c0 + j] = sm[j * kThreads + tid];
    }
}

// Second level: block b owns columns 32 b .. 32 b + 31; group g of its threads adds records g, g + 8, ... in that order, then the
// 8 groups are folded by a fixed tree.  No record (nrows == 0): zeros.
__global__ __launch_bounds__(kThreads) void finalize_kernel(const double *__restrict__ ws, int64_t nbands, int f, float *__restrict__ dbias) {
    __shared__ double sm[kThreads];
    const int tid = threadIdx.x, lane = tid & (kFinalCols - 1), grp = tid / kFinalCols;
    const int o = blockIdx.x * kFinalCols + lane;
    double acc = 0.0;
    if (o < f)
        for (int64_t b = grp; b < nbands; b += kFinalGroups) acc += ws[b * (int64_t)f + o];
    sm[tid] = acc;
    for (int s = kFinalGroups >> 1; s >= 1; s >>= 1) {
        __syncthreads();
        if (grp < s) sm[tid] += sm[tid + s * kFinalCols];
    }
    if (grp == 0 && o < f) dbias[o] = (float)sm[tid];
}

int log2_threads_per_row(int f) {
    const int quads = (f + 3) / 4;
    int l = 0;
    while ((1 << l) < quads) ++l;
    return l;
}

bool aligned16(const void *p) { return ((uintptr_t)p % 16) == 0; }
bool rows16(int64_t ld) { return ld % 4 == 0; }
int64_t bands(int64_t nrows) { return (nrows + kSumRows - 1) / kSumRows; }

DropArgs drop_args(const int64_t *row_ids, uint64_t seed, const int64_t *step, uint32_t layer, uint32_t thr) {
#pragma clang fp contract(off)
    DropArgs a;
    a.row_ids = row_ids;
    a.step = thr > 0 ? step : nullptr;     // (thr == 0 keeps everything at scale 1: the path without dropout, bit for bit)
    a.seed = seed;
    a.layer = layer;
    a.thr = thr;
    a.scale = dropout_scale(thr);
    a.inv_scale = 1.0f / a.scale;
    return a;
}

}  // namespace

extern "C" int64_t pgcn_gat_tail_ws_bytes(int64_t nrows, int32_t fout) {
    if (nrows < 0 || fout < 1 || fout > kMaxF) return -1;
    const int64_t nb = bands(nrows);
    return (nb > 0 ? nb : 1) * (int64_t)fout * (int64_t)sizeof(double);
}

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
    const int l2 = log2_threads_per_row(f);
    const int64_t nb = (nrows + kApplyRows - 1) / kApplyRows;
    const bool vec = f % 4 == 0 && rows16(ldx) && rows16(ldy) && aligned16(X) && aligned16(Y);
    if (vec)
        hipLaunchKernelGGL(forward_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, X, ldx, bias, nrows, f, nsum,
                           inv_heads, l2, (int)act, da, Y, ldy);
    else
        hipLaunchKernelGGL(forward_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, X, ldx, bias, nrows, f, nsum,
                           inv_heads, l2, (int)act, da, Y, ldy);
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
        if (vec)
            hipLaunchKernelGGL(backward_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, s, G, ldg, Y, ldy, nrows, f, nsum, inv_heads, l2,
                               (int)act, da, dX, lddx, rec);
        else
            hipLaunchKernelGGL(backward_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, s, G, ldg, Y, ldy, nrows, f, nsum, inv_heads, l2,
                               (int)act, da, dX, lddx, rec);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    if (dbias) {
        hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((f + kFinalCols - 1) / kFinalCols)), dim3(kThreads), 0, s, (const double *)ws, nb,
                           f, dbias);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    return PGCN_OK;
}
