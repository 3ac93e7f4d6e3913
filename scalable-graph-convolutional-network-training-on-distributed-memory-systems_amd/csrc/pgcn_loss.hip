// pgcn_loss.hip -- row-wise negative log-likelihood of a log-softmax, forward and backward, for gfx950.
//
//   loss_i = logsumexp_j x_ij - x_i,label_i            replaces F.nll_loss(F.log_softmax(logits, 1), labels)
//   dx_ij  = g * (exp(x_ij - lse_i) - [j == label_i])     /root/reference/GPU/PGCN.py:214-215 and its autograd graph
//
// The framework composes this from ~12 element-wise / reduction launches over the n x f logits (0.6 ms of a
// 13 ms epoch at the benchmark size); here it is one pass each way: a wave owns a row (f <= 64 * 16 = 1024
// columns, lane j takes columns j, j + 64, ...), maximum and sum by butterfly shuffles, fixed order =>
// bit-reproducible.  HBM-bound streams: 4 f bytes per row forward, 8 f bytes per row backward.
//
// Masked variant for node classification (pgcn_masked_nll_f32 / _backward_f32): every row carries a split code (0 in no set,
// 1 train, 2 val, 3 test).  ONE pass over the logits leaves lse_i for every row and, per set, the sum of the row losses, the
// number of rows whose arg-max (lowest index among equal maxima) is the label, and the number of rows: the training loss and the
// three accuracies of a step without logits[mask] (a host synchronisation), without an argmax / eq / sum chain per set.  A block
// owns 64 consecutive rows and writes one partial record; a second, one-block launch adds the records (pgcn_setrecord.h: the
// record, the fixed order of its sums and what that promises).  4 C + 9 bytes per row forward; the backward writes g (softmax - onehot)
// on train rows and zeros elsewhere, and reads the logits of train rows only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"
#include "pgcn_setrecord.h"

namespace {

constexpr int kMaxPerLane = 16;

__device__ __forceinline__ float wsum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wmax(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(kThreads) void nll_rows_kernel(const float *__restrict__ X, int64_t ldx,
                                                            const int64_t *__restrict__ labels, int64_t nrows, int32_t f,
                                                            float *__restrict__ loss, float *__restrict__ lse) {
    const int64_t i = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= nrows) return;
    const float *x = X + i * ldx;
    float v[kMaxPerLane];
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < kMaxPerLane; ++q) {
        const int j = lane + 64 * q;
        v[q] = j < f ? x[j] : -INFINITY;
        m = fmaxf(m, v[q]);
    }
    m = wmax(m);
    const float mm = isinf(m) ? 0.f : m;               // like torch.logsumexp: an all -inf (or +inf) row must not make NaN
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < kMaxPerLane; ++q) s += (lane + 64 * q < f) ? expf(v[q] - mm) : 0.f;
    s = wsum(s);
    const float l = logf(s) + mm;
    if (lane == 0) {
        const int64_t y = labels[i];
        lse[i] = l;
        // a label outside [0, f) poisons the row's loss with NaN (F.nll_loss raises; no out-of-bounds read here)
        loss[i] = (y >= 0 && y < f) ? l - x[y] : __builtin_nanf("");
    }
}

__global__ __launch_bounds__(kThreads) void nll_rows_backward_kernel(const float *__restrict__ X, int64_t ldx,
                                                                     const int64_t *__restrict__ labels,
                                                                     const float *__restrict__ lse,
                                                                     const float *__restrict__ gscale, float scale,
                                                                     int64_t nrows, int32_t f, float *__restrict__ dX,
                                                                     int64_t lddx) {
    const int64_t i = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= nrows) return;
    const float g = (gscale ? gscale[0] : 1.f) * scale;
    const float l = lse[i];
    const int64_t y = labels[i];
    const float *x = X + i * ldx;
    float *dx = dX + i * lddx;
    for (int j = lane; j < f; j += 64) dx[j] = g * (expf(x[j] - l) - (j == y ? 1.f : 0.f));
}

// f % 4 == 0, f <= 256, 16-byte aligned rows (the shapes of the training loops): 16 lanes own a row (float4 chunks
// c = sub, sub + 16, ...), four rows per wave -- a wave keeps 4 x more bytes in flight than with a row per wave (the
// kernel is a latency chain per row: 114 -> see DESIGN 6 at the benchmark size).  Fixed order => bit-reproducible.
constexpr int kV4Chunks = 4;

__device__ __forceinline__ float gsum16(float v) {
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float gmax16(float v) {
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(kThreads) void nll_rows_v4_kernel(const float *__restrict__ X, int64_t ldx,
                                                               const int64_t *__restrict__ labels, int64_t nrows, int32_t f,
                                                               float *__restrict__ loss, float *__restrict__ lse) {
    const int lane = threadIdx.x & 63, sub = lane & 15;
    const int64_t i = ((int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) * 4 + (lane >> 4);
    const bool act = i < nrows;
    const float4 *x4 = reinterpret_cast<const float4 *>(X + (act ? i : 0) * ldx);
    const int nch = f >> 2;
    float4 v[kV4Chunks];
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < kV4Chunks; ++q) {
        const int c = sub + 16 * q;
        if (act && c < nch) {
            v[q] = x4[c];
            m = fmaxf(fmaxf(fmaxf(m, v[q].x), fmaxf(v[q].y, v[q].z)), v[q].w);
        } else {
            v[q] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        }
    }
    m = gmax16(m);
    const float mm = isinf(m) ? 0.f : m;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < kV4Chunks; ++q)
        if (sub + 16 * q < nch) s += (expf(v[q].x - mm) + expf(v[q].y - mm)) + (expf(v[q].z - mm) + expf(v[q].w - mm));
    s = gsum16(s);
    const float l = logf(s) + mm;
    if (act && sub == 0) {
        const int64_t y = labels[i];
        lse[i] = l;
        loss[i] = (y >= 0 && y < f) ? l - X[i * ldx + y] : __builtin_nanf("");
    }
}

__global__ __launch_bounds__(kThreads) void nll_rows_backward_v4_kernel(const float *__restrict__ X, int64_t ldx,
                                                                        const int64_t *__restrict__ labels,
                                                                        const float *__restrict__ lse,
                                                                        const float *__restrict__ gscale, float scale,
                                                                        int64_t nrows, int32_t f, float *__restrict__ dX,
                                                                        int64_t lddx) {
    const int lane = threadIdx.x & 63, sub = lane & 15;
    const int64_t i = ((int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) * 4 + (lane >> 4);
    if (i >= nrows) return;
    const float g = (gscale ? gscale[0] : 1.f) * scale;
    const float l = lse[i];
    const int y = (int)labels[i];
    const float4 *x4 = reinterpret_cast<const float4 *>(X + i * ldx);
    float4 *d4 = reinterpret_cast<float4 *>(dX + i * lddx);
    const int nch = f >> 2;
    for (int c = sub; c < nch; c += 16) {
        const float4 x = x4[c];
        const int j = 4 * c;
        d4[c] = make_float4(g * (expf(x.x - l) - (j == y ? 1.f : 0.f)), g * (expf(x.y - l) - (j + 1 == y ? 1.f : 0.f)),
                            g * (expf(x.z - l) - (j + 2 == y ? 1.f : 0.f)), g * (expf(x.w - l) - (j + 3 == y ? 1.f : 0.f)));
    }
}

// ---- masked loss + accuracy ------------------------------------------------------------------------------------------------------
using NllRecord = SetRecord<1>;          // pgcn_masked_nll_stats: double loss_sum[4], int64 correct[4], int64 rows[4]
static_assert(sizeof(pgcn_masked_nll_stats) == NllRecord::kWords * sizeof(unsigned long long), "record layout");
constexpr int kNoColumn = 0x7fffffff;

// the row's part of the statistics, by the lane that leads the row.  Labels of rows in no set are not read.
__device__ __forceinline__ void masked_row(NllRecord &acc, const float *__restrict__ X, int64_t ldx, const int64_t *__restrict__ labels,
                                           const uint8_t *__restrict__ split, int64_t i, int32_t f, float l, int best) {
    const int k = split_code(split, i);
    float nll = 0.f;
    bool hit = false;
    if (k != 0) {
        const int64_t y = labels[i];
        const bool valid = y >= 0 && y < f;
        // a label outside [0, f): NaN in this set's sum, the row counts as wrong, nothing is read through it
        nll = valid ? l - X[i * ldx + y] : __builtin_nanf("");
        hit = valid && (int64_t)best == y;
    }
    const int c[1] = {hit ? 1 : 0};
    acc.add(k, nll, c);
}

// general widths: a wave owns a row (lane j takes columns j, j + 64, ...; Q of them), 4 rows per step, 16 steps per block
template <int Q>
__global__ __launch_bounds__(kThreads) void masked_nll_kernel(const float *__restrict__ X, int64_t ldx,
                                                              const int64_t *__restrict__ labels,
                                                              const uint8_t *__restrict__ split, int64_t nrows, int32_t f,
                                                              float *__restrict__ lse, unsigned long long *__restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    NllRecord acc;
    acc.clear();
#pragma unroll 4
    for (int it = 0; it < kSetRows / 4; ++it) {
        const int64_t i = (int64_t)blockIdx.x * kSetRows + it * 4 + wave;
        if (i >= nrows) break;                            // (wave-uniform)
        const float *x = X + i * ldx;
        float v[Q];
        float m = -INFINITY;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int j = lane + 64 * q;
            v[q] = j < f ? x[j] : -INFINITY;
            m = fmaxf(m, v[q]);
        }
        m = wmax(m);
        const float mm = isinf(m) ? 0.f : m;
        float s = 0.f;
        int best = kNoColumn;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int j = lane + 64 * q;
            s += j < f ? expf(v[q] - mm) : 0.f;
            best = min(best, (j < f && v[q] == m) ? j : kNoColumn);
        }
        s = wsum(s);
        for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
        const float l = logf(s) + mm;
        if (lane == 0) {
            lse[i] = l;
            masked_row(acc, X, ldx, labels, split, i, f, l, best);
        }
    }
    acc.block_store(part);
}

// f % 4 == 0, f <= 256, 16-byte aligned rows: 16 lanes own a row (CH float4 chunks each), 16 rows per step, 4 steps per block
template <int CH>
__global__ __launch_bounds__(kThreads) void masked_nll_v4_kernel(const float *__restrict__ X, int64_t ldx,
                                                                 const int64_t *__restrict__ labels,
                                                                 const uint8_t *__restrict__ split, int64_t nrows, int32_t f,
                                                                 float *__restrict__ lse, unsigned long long *__restrict__ part) {
    const int lane = threadIdx.x & 63, sub = lane & 15;
    const int nch = f >> 2;
    NllRecord acc;
    acc.clear();
#pragma unroll
    for (int it = 0; it < kSetRows / 16; ++it) {
        const int64_t i = (int64_t)blockIdx.x * kSetRows + it * 16 + (threadIdx.x >> 6) * 4 + (lane >> 4);
        const bool act = i < nrows;
        const float4 *x4 = reinterpret_cast<const float4 *>(X + (act ? i : 0) * ldx);
        float4 v[CH];
        float m = -INFINITY;
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const int c = sub + 16 * q;
            if (act && c < nch) {
                v[q] = x4[c];
                m = fmaxf(fmaxf(fmaxf(m, v[q].x), fmaxf(v[q].y, v[q].z)), v[q].w);
            } else {
                v[q] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            }
        }
        m = gmax16(m);
        const float mm = isinf(m) ? 0.f : m;
        float s = 0.f;
        int best = kNoColumn;
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const int c = sub + 16 * q;
            if (c < nch) {
                s += (expf(v[q].x - mm) + expf(v[q].y - mm)) + (expf(v[q].z - mm) + expf(v[q].w - mm));
                const int j = 4 * c;
                const int b = v[q].x == m ? j : v[q].y == m ? j + 1 : v[q].z == m ? j + 2 : v[q].w == m ? j + 3 : kNoColumn;
                best = min(best, b);
            }
        }
        s = gsum16(s);
        for (int o = 8; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
        const float l = logf(s) + mm;
        if (act && sub == 0) {
            lse[i] = l;
            masked_row(acc, X, ldx, labels, split, i, f, l, best);
        }
    }
    acc.block_store(part);
}

__global__ __launch_bounds__(kThreads) void masked_nll_backward_kernel(const float *__restrict__ X, int64_t ldx,
                                                                       const int64_t *__restrict__ labels,
                                                                       const uint8_t *__restrict__ split,
                                                                       const float *__restrict__ lse,
                                                                       const float *__restrict__ gscale, float scale,
                                                                       int64_t nrows, int32_t f, float *__restrict__ dX,
                                                                       int64_t lddx) {
    const int64_t i = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= nrows) return;
    float *dx = dX + i * lddx;
    if (split[i] != 1) {                                  // not a train row: exact zeros, its logits are not read
        for (int j = lane; j < f; j += 64) dx[j] = 0.f;
        return;
    }
    const float g = (gscale ? gscale[0] : 1.f) * scale;
    const float l = lse[i];
    const int64_t y = labels[i];
    const float *x = X + i * ldx;
    for (int j = lane; j < f; j += 64) dx[j] = g * (expf(x[j] - l) - (j == y ? 1.f : 0.f));
}

__global__ __launch_bounds__(kThreads) void masked_nll_backward_v4_kernel(const float *__restrict__ X, int64_t ldx,
                                                                          const int64_t *__restrict__ labels,
                                                                          const uint8_t *__restrict__ split,
                                                                          const float *__restrict__ lse,
                                                                          const float *__restrict__ gscale, float scale,
                                                                          int64_t nrows, int32_t f, float *__restrict__ dX,
                                                                          int64_t lddx) {
    const int lane = threadIdx.x & 63, sub = lane & 15;
    const int64_t i = ((int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) * 4 + (lane >> 4);
    if (i >= nrows) return;
    float4 *d4 = reinterpret_cast<float4 *>(dX + i * lddx);
    const int nch = f >> 2;
    if (split[i] != 1) {
        for (int c = sub; c < nch; c += 16) d4[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float g = (gscale ? gscale[0] : 1.f) * scale;
    const float l = lse[i];
    const int64_t y64 = labels[i];
    const int y = (y64 >= 0 && y64 < f) ? (int)y64 : -1;
    const float4 *x4 = reinterpret_cast<const float4 *>(X + i * ldx);
    for (int c = sub; c < nch; c += 16) {
        const float4 x = x4[c];
        const int j = 4 * c;
        d4[c] = make_float4(g * (expf(x.x - l) - (j == y ? 1.f : 0.f)), g * (expf(x.y - l) - (j + 1 == y ? 1.f : 0.f)),
                            g * (expf(x.z - l) - (j + 2 == y ? 1.f : 0.f)), g * (expf(x.w - l) - (j + 3 == y ? 1.f : 0.f)));
    }
}

}  // namespace

extern "C" int pgcn_nll_rows_f32(const float *X, int64_t ldx, const int64_t *labels, int64_t nrows, int32_t f,
                                 float *loss_rows, float *lse_rows, pgcn_stream_t stream) {
    if (nrows < 0 || f <= 0 || ldx < f) return pgcn_set_error(PGCN_EINVAL, "pgcn_nll_rows_f32: bad sizes");
    if (f > 64 * kMaxPerLane) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_nll_rows_f32: more than 1024 columns");
    if (nrows == 0) return PGCN_OK;
    if (!X || !labels || !loss_rows || !lse_rows) return pgcn_set_error(PGCN_EINVAL, "pgcn_nll_rows_f32: null pointer");
    if (f % 4 == 0 && f <= 64 * kV4Chunks && ldx % 4 == 0 && (uintptr_t)X % 16 == 0) {
        const int64_t g4 = (nrows + 15) / 16;
        if (g4 > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_nll_rows_f32: too many rows");
        hipLaunchKernelGGL(nll_rows_v4_kernel, dim3((unsigned)g4), dim3(kThreads), 0, (hipStream_t)stream, X, ldx, labels, nrows,
                           f, loss_rows, lse_rows);
        PGCN_HIP_CHECK(hipGetLastError());
        return PGCN_OK;
    }
    const int64_t grid = (nrows + 3) / 4;
    if (grid > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_nll_rows_f32: too many rows");
    hipLaunchKernelGGL(nll_rows_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, X, ldx, labels, nrows,
                       f, loss_rows, lse_rows);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_nll_rows_backward_f32(const float *X, int64_t ldx, const int64_t *labels, const float *lse_rows,
                                          const float *gscale_dev, float scale, int64_t nrows, int32_t f, float *dX,
                                          int64_t lddx, pgcn_stream_t stream) {
    if (nrows < 0 || f <= 0 || ldx < f || lddx < f) return pgcn_set_error(PGCN_EINVAL, "pgcn_nll_rows_backward_f32: bad sizes");
    if (nrows == 0) return PGCN_OK;
    if (!X || !labels || !lse_rows || !dX) return pgcn_set_error(PGCN_EINVAL, "pgcn_nll_rows_backward_f32: null pointer");
    if (f % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)dX % 16 == 0) {
        const int64_t g4 = (nrows + 15) / 16;
        if (g4 > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_nll_rows_backward_f32: too many rows");
        hipLaunchKernelGGL(nll_rows_backward_v4_kernel, dim3((unsigned)g4), dim3(kThreads), 0, (hipStream_t)stream, X, ldx,
                           labels, lse_rows, gscale_dev, scale, nrows, f, dX, lddx);
        PGCN_HIP_CHECK(hipGetLastError());
        return PGCN_OK;
    }
    const int64_t grid = (nrows + 3) / 4;
    if (grid > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_nll_rows_backward_f32: too many rows");
    hipLaunchKernelGGL(nll_rows_backward_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, X, ldx, labels,
                       lse_rows, gscale_dev, scale, nrows, f, dX, lddx);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int64_t pgcn_masked_nll_ws_bytes(int64_t nrows) { return set_ws_bytes<1>(nrows); }

extern "C" int pgcn_masked_nll_f32(const float *X, int64_t ldx, const int64_t *labels, const uint8_t *split, int64_t nrows,
                                   int32_t C, float *lse_rows, pgcn_masked_nll_stats *stats, void *ws, int64_t ws_bytes,
                                   pgcn_stream_t stream) {
    if (nrows < 0 || C <= 0 || ldx < C) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_nll_f32: bad sizes");
    if (C > 64 * kMaxPerLane) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_masked_nll_f32: more than 1024 columns");
    int64_t blocks;
    if (int rc = set_check_record("pgcn_masked_nll_f32", stats, nrows, &blocks)) return rc;
    unsigned long long *part = static_cast<unsigned long long *>(ws);
    if (nrows > 0) {
        if (!X || !labels || !split || !lse_rows) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_nll_f32: null pointer");
        if (int rc = set_check_ws<1>("pgcn_masked_nll_f32", ws, ws_bytes, nrows)) return rc;
        const dim3 grid((unsigned)blocks), block(kThreads);
        hipStream_t st = (hipStream_t)stream;
#define PGCN_MASKED_LAUNCH(kernel) hipLaunchKernelGGL(kernel, grid, block, 0, st, X, ldx, labels, split, nrows, C, lse_rows, part)
        if (C % 4 == 0 && C <= 64 * kV4Chunks && ldx % 4 == 0 && (uintptr_t)X % 16 == 0) {
            if (C <= 64) PGCN_MASKED_LAUNCH(masked_nll_v4_kernel<1>);
            else if (C <= 128) PGCN_MASKED_LAUNCH(masked_nll_v4_kernel<2>);
            else PGCN_MASKED_LAUNCH(masked_nll_v4_kernel<4>);
        } else {
            if (C <= 64) PGCN_MASKED_LAUNCH(masked_nll_kernel<1>);
            else if (C <= 128) PGCN_MASKED_LAUNCH(masked_nll_kernel<2>);
            else if (C <= 256) PGCN_MASKED_LAUNCH(masked_nll_kernel<4>);
            else PGCN_MASKED_LAUNCH(masked_nll_kernel<kMaxPerLane>);
        }
#undef PGCN_MASKED_LAUNCH
        PGCN_HIP_CHECK(hipGetLastError());
    }
    return set_finalize<1>(ws, blocks, stats, stream);
}

extern "C" int pgcn_masked_nll_backward_f32(const float *X, int64_t ldx, const int64_t *labels, const uint8_t *split,
                                            const float *lse_rows, const float *gscale_dev, float scale, int64_t nrows, int32_t C,
                                            float *dX, int64_t lddx, pgcn_stream_t stream) {
    if (nrows < 0 || C <= 0 || ldx < C || lddx < C) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_nll_backward_f32: bad sizes");
    if (C > 64 * kMaxPerLane) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_masked_nll_backward_f32: more than 1024 columns");
    if (nrows == 0) return PGCN_OK;
    if (!X || !labels || !split || !lse_rows || !dX) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_nll_backward_f32: null pointer");
    if (C % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)dX % 16 == 0) {
        const int64_t g4 = (nrows + 15) / 16;
        if (g4 > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_nll_backward_f32: too many rows");
        hipLaunchKernelGGL(masked_nll_backward_v4_kernel, dim3((unsigned)g4), dim3(kThreads), 0, (hipStream_t)stream, X, ldx,
                           labels, split, lse_rows, gscale_dev, scale, nrows, C, dX, lddx);
        PGCN_HIP_CHECK(hipGetLastError());
        return PGCN_OK;
    }
    const int64_t grid = (nrows + 3) / 4;
    if (grid > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_nll_backward_f32: too many rows");
    hipLaunchKernelGGL(masked_nll_backward_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, X, ldx, labels,
                       split, lse_rows, gscale_dev, scale, nrows, C, dX, lddx);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}
