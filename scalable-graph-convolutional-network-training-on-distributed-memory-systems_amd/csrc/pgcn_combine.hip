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
// Layout as in pgcn_norm.hip: 256 threads; a thread owns FOUR consecutive columns, TPR = the power of two >= ceil(f / 4) threads
// span a row, 256 / TPR row groups walk a band of consecutive rows, four rows per thread in flight; the bias and the column's
// share of the dropout hash are loaded / formed once per thread, before the row loop.  f <= 1024.  One float4 per thread and row
// when f % 4 == 0 and every base and leading dimension keeps the rows 16-byte aligned, four guarded scalars otherwise: the same
// thread does the same arithmetic in the same order, so both paths leave the same bits (contraction is off in every body).
//
// dbias: a block of the backward owns kSumRows consecutive rows; its threads add Gm in double registers, the row groups are
// folded through LDS by a fixed tree, the block writes ONE partial record [f] of doubles to the work-space; the second launch
// gives each block 32 columns, 8 groups of threads add the records b = group, group + 8, ... in that order and a fixed tree folds
// the 8 -- no floating-point atomics, the same input gives the same bits.  No thread touches two columns' sums: a NaN or inf stays
// in its own column.  Raw pointers + a stream, no allocation, no synchronisation: graph-capturable.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"

#define PG_DROPOUT_FN __host__ __device__ __forceinline__
#include "../gemm/pgcn_dropout.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSumRows = 512;      // rows of a block of the backward (kernels.COMBINE_SUM_ROWS restates it)
constexpr int kApplyRows = 128;    // rows of a block of the forward
constexpr int kFinalCols = 32;     // columns of a block of the second level
constexpr int kFinalGroups = kThreads / kFinalCols;
constexpr int kMaxF = 1024;

struct Quad {
    float v[4];
};

// (no __restrict__ on the matrices: Y may be Z1 itself; a thread reads its own elements before it writes them)
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

struct DropArgs {
    const int64_t *row_ids;
    const int64_t *step;       // NULL: no dropout
    uint64_t seed;
    uint32_t layer, thr;
    float scale;
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void forward_kernel(const float *Z1, int64_t ldz1, const float *Z2, int64_t ldz2,
                                                           const float *__restrict__ bias, int64_t nrows, int f, int log2_tpr, int do_relu,
                                                           DropArgs d, float *Y, int64_t ldy) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, u = tid & ((1 << log2_tpr) - 1), rg = tid >> log2_tpr, ngroups = kThreads >> log2_tpr;
    const int c0 = 4 * u;
    if (c0 >= f) return;
    const int64_t r0 = (int64_t)blockIdx.x * kApplyRows;
    const int64_t rend = r0 + kApplyRows < nrows ? r0 + kApplyRows : nrows;
    const bool has_z2 = Z2 != nullptr, has_bias = bias != nullptr;
    float b[4] = {0.f, 0.f, 0.f, 0.f};
    if (has_bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = c0 + j < f ? bias[c0 + j] : 0.f;
    }
    const bool drop = do_relu && d.step != nullptr;
    uint64_t key = 0;
    uint32_t dcol[4] = {0, 0, 0, 0};
    if (drop) {
        key = dropout_key(d.seed, (uint64_t)d.step[0], d.layer);
#pragma unroll
        for (int j = 0; j < 4; ++j) dcol[j] = dropout_col(key, (uint32_t)(c0 + j));      // the column's share: once per column
    }
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

// One pass over G (and Y): writes Gm (Gm != NULL) and, when ws != NULL, the band's column sums of Gm in double.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void backward_kernel(const float *G, int64_t ldg, const float *__restrict__ Y, int64_t ldy,
                                                            int64_t nrows, int f, int log2_tpr, int do_relu, float scale, float *Gm,
                                                            int64_t ldgm, double *__restrict__ ws) {
#pragma clang fp contract(off)
    __shared__ double sm[4 * kThreads];
    const int tid = threadIdx.x, u = tid & ((1 << log2_tpr) - 1), rg = tid >> log2_tpr, ngroups = kThreads >> log2_tpr;
    const int c0 = 4 * u;
    const bool active = c0 < f;
    const int64_t r0 = (int64_t)blockIdx.x * kSumRows;
    const int64_t rend = r0 + kSumRows < nrows ? r0 + kSumRows : nrows;
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

}  // namespace

extern "C" int64_t pgcn_combine_ws_bytes(int64_t nrows, int32_t f) {
    if (nrows < 0 || f < 1 || f > kMaxF) return -1;
    const int64_t nb = bands(nrows);
    return (nb > 0 ? nb : 1) * (int64_t)f * (int64_t)sizeof(double);
}

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
    DropArgs d;
    d.row_ids = row_ids;
    d.step = (relu && thr > 0) ? step : nullptr;   // (thr == 0 keeps everything at scale 1: the path without dropout, bit for bit)
    d.seed = seed;
    d.layer = layer;
    d.thr = thr;
    d.scale = dropout_scale(thr);
    const int l2 = log2_threads_per_row(f);
    const int64_t nb = (nrows + kApplyRows - 1) / kApplyRows;
    const bool vec = f % 4 == 0 && rows16(ldz1) && rows16(ldy) && aligned16(Z1) && aligned16(Y) && (!Z2 || (rows16(ldz2) && aligned16(Z2)));
    if (vec)
        hipLaunchKernelGGL(forward_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, Z1, ldz1, Z2, ldz2, bias, nrows,
                           (int)f, l2, (int)(relu != 0), d, Y, ldy);
    else
        hipLaunchKernelGGL(forward_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, Z1, ldz1, Z2, ldz2, bias, nrows,
                           (int)f, l2, (int)(relu != 0), d, Y, ldy);
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
        if (vec)
            hipLaunchKernelGGL(backward_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, s, G, ldg, Y, ldy, nrows, (int)f, l2,
                               (int)(relu != 0), scale, Gm, ldgm, rec);
        else
            hipLaunchKernelGGL(backward_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, s, G, ldg, Y, ldy, nrows, (int)f, l2,
                               (int)(relu != 0), scale, Gm, ldgm, rec);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    if (dbias) {
        hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((f + kFinalCols - 1) / kFinalCols)), dim3(kThreads), 0, s, (const double *)ws, nb,
                           (int)f, dbias);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    return PGCN_OK;
}
