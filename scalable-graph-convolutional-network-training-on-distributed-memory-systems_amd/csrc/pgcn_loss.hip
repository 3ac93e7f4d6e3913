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
// owns 64 consecutive rows and writes one partial record; a second, one-block launch adds the records in block order -- no
// floating-point atomics, two calls give the same bits.  4 C + 9 bytes per row forward; the backward writes g (softmax - onehot)
// on train rows and zeros elsewhere, and reads the logits of train rows only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"

namespace {

constexpr int kThreads = 256;
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
constexpr int kMaskedRows = 64;          // rows per block of the forward: one partial record per 64 rows
constexpr int kStatWords = 12;           // pgcn_masked_nll_stats: double loss_sum[4], int64 correct[4], int64 rows[4]
constexpr int kNoColumn = 0x7fffffff;

// what one lane has seen of the rows it leads (slot 0 = rows in no set: counted, nothing else)
struct SetAcc {
    double loss[3];
    int correct[3];
    int rows[4];
    __device__ __forceinline__ void clear() {
        loss[0] = loss[1] = loss[2] = 0.0;
        correct[0] = correct[1] = correct[2] = 0;
        rows[0] = rows[1] = rows[2] = rows[3] = 0;
    }
    // selects, not products: a NaN row loss reaches its own set only
    __device__ __forceinline__ void add(int k, float nll, bool hit) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            loss[s] += (k == s + 1) ? (double)nll : 0.0;
            correct[s] += (k == s + 1 && hit) ? 1 : 0;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) rows[s] += (k == s) ? 1 : 0;
    }
};

// the row's part of the statistics, by the lane that leads the row.  Labels of rows in no set are not read.
__device__ __forceinline__ void masked_row(SetAcc &acc, const float *__restrict__ X, int64_t ldx, const int64_t *__restrict__ labels,
                                           const uint8_t *__restrict__ split, int64_t i, int32_t f, float l, int best) {
    const int s = split[i];
    const int k = s <= 3 ? s : 0;
    float nll = 0.f;
    bool hit = false;
    if (k != 0) {
        const int64_t y = labels[i];
        const bool valid = y >= 0 && y < f;
        // a label outside [0, f): NaN in this set's sum, the row counts as wrong, nothing is read through it
        nll = valid ? l - X[i * ldx + y] : __builtin_nanf("");
        hit = valid && (int64_t)best == y;
    }
    acc.add(k, nll, hit);
}

// butterfly over the wave, then the block's four waves in order: one record per block, fixed order
__device__ __forceinline__ void masked_block_store(SetAcc &acc, unsigned long long *__restrict__ part) {
    __shared__ double s_loss[kThreads / 64][3];
    __shared__ int s_cnt[kThreads / 64][7];
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            acc.loss[s] += __shfl_xor(acc.loss[s], o, 64);
            acc.correct[s] += __shfl_xor(acc.correct[s], o, 64);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc.rows[s] += __shfl_xor(acc.rows[s], o, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int s = 0; s < 3; ++s) {
            s_loss[w][s] = acc.loss[s];
            s_cnt[w][s] = acc.correct[s];
        }
        for (int s = 0; s < 4; ++s) s_cnt[w][3 + s] = acc.rows[s];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *pl = reinterpret_cast<double *>(part + (size_t)blockIdx.x * kStatWords);
        long long *pc = reinterpret_cast<long long *>(part + (size_t)blockIdx.x * kStatWords) + 4;
        pl[0] = 0.0;
        pc[0] = 0;
        for (int s = 0; s < 3; ++s) {
            double a = s_loss[0][s];
            long long c = s_cnt[0][s];
            for (int v = 1; v < kThreads / 64; ++v) {
                a += s_loss[v][s];
                c += s_cnt[v][s];
            }
            pl[1 + s] = a;
            pc[1 + s] = c;
        }
        for (int s = 0; s < 4; ++s) {
            long long c = s_cnt[0][3 + s];
            for (int v = 1; v < kThreads / 64; ++v) c += s_cnt[v][3 + s];
            pc[4 + s] = c;
        }
    }
}

// general widths: a wave owns a row (lane j takes columns j, j + 64, ...; Q of them), 4 rows per step, 16 steps per block
template <int Q>
__global__ __launch_bounds__(kThreads) void masked_nll_kernel(const float *__restrict__ X, int64_t ldx,
                                                              const int64_t *__restrict__ labels,
                                                              const uint8_t *__restrict__ split, int64_t nrows, int32_t f,
                                                              float *__restrict__ lse, unsigned long long *__restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    SetAcc acc;
    acc.clear();
#pragma unroll 4
    for (int it = 0; it < kMaskedRows / 4; ++it) {
        const int64_t i = (int64_t)blockIdx.x * kMaskedRows + it * 4 + wave;
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
    masked_block_store(acc, part);
}

// f % 4 == 0, f <= 256, 16-byte aligned rows: 16 lanes own a row (CH float4 chunks each), 16 rows per step, 4 steps per block
template <int CH>
__global__ __launch_bounds__(kThreads) void masked_nll_v4_kernel(const float *__restrict__ X, int64_t ldx,
                                                                 const int64_t *__restrict__ labels,
                                                                 const uint8_t *__restrict__ split, int64_t nrows, int32_t f,
                                                                 float *__restrict__ lse, unsigned long long *__restrict__ part) {
    const int lane = threadIdx.x & 63, sub = lane & 15;
    const int nch = f >> 2;
    SetAcc acc;
    acc.clear();
#pragma unroll
    for (int it = 0; it < kMaskedRows / 16; ++it) {
        const int64_t i = (int64_t)blockIdx.x * kMaskedRows + it * 16 + (threadIdx.x >> 6) * 4 + (lane >> 4);
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
    masked_block_store(acc, part);
}

// one block: thread t adds records t, t + 256, ... in that order, then the same butterfly / wave order as above
__global__ __launch_bounds__(kThreads) void masked_nll_finalize_kernel(const unsigned long long *__restrict__ part, int64_t nblocks,
                                                                       unsigned long long *__restrict__ stats) {
    __shared__ double s_loss[kThreads / 64][3];
    __shared__ long long s_cnt[kThreads / 64][7];
    double loss[3] = {0.0, 0.0, 0.0};
    long long cnt[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int64_t b = threadIdx.x; b < nblocks; b += kThreads) {
        const double *pl = reinterpret_cast<const double *>(part + b * kStatWords);
        const long long *pc = reinterpret_cast<const long long *>(part + b * kStatWords) + 4;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            loss[s] += pl[1 + s];
            cnt[s] += pc[1 + s];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) cnt[3 + s] += pc[4 + s];
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int s = 0; s < 3; ++s) loss[s] += __shfl_xor(loss[s], o, 64);
#pragma unroll
        for (int s = 0; s < 7; ++s) cnt[s] += __shfl_xor(cnt[s], o, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int s = 0; s < 3; ++s) s_loss[w][s] = loss[s];
        for (int s = 0; s < 7; ++s) s_cnt[w][s] = cnt[s];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *ol = reinterpret_cast<double *>(stats);
        long long *oc = reinterpret_cast<long long *>(stats) + 4;
        ol[0] = 0.0;
        oc[0] = 0;
        for (int s = 0; s < 3; ++s) {
            double a = s_loss[0][s];
            for (int v = 1; v < kThreads / 64; ++v) a += s_loss[v][s];
            ol[1 + s] = a;
        }
        for (int s = 0; s < 7; ++s) {
            long long c = s_cnt[0][s];
            for (int v = 1; v < kThreads / 64; ++v) c += s_cnt[v][s];
            oc[1 + s] = c;                                // correct[1..3], then rows[0..3]
        }
    }
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

extern "C" int64_t pgcn_masked_nll_ws_bytes(int64_t nrows) {
    const int64_t blocks = nrows > 0 ? (nrows + kMaskedRows - 1) / kMaskedRows : 1;
    return blocks * kStatWords * (int64_t)sizeof(unsigned long long);
}

extern "C" int pgcn_masked_nll_f32(const float *X, int64_t ldx, const int64_t *labels, const uint8_t *split, int64_t nrows,
                                   int32_t C, float *lse_rows, pgcn_masked_nll_stats *stats, void *ws, int64_t ws_bytes,
                                   pgcn_stream_t stream) {
    if (nrows < 0 || C <= 0 || ldx < C) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_nll_f32: bad sizes");
    if (C > 64 * kMaxPerLane) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_masked_nll_f32: more than 1024 columns");
    if (!stats || (uintptr_t)stats % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_nll_f32: stats must be 8-byte aligned");
    const int64_t blocks = (nrows + kMaskedRows - 1) / kMaskedRows;
    if (blocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_nll_f32: too many rows");
    unsigned long long *part = static_cast<unsigned long long *>(ws);
    if (nrows > 0) {
        if (!X || !labels || !split || !lse_rows) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_nll_f32: null pointer");
        if (!ws || (uintptr_t)ws % 8 != 0 || ws_bytes < pgcn_masked_nll_ws_bytes(nrows))
            return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_nll_f32: work-space too small or not 8-byte aligned");
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
    // (no rows: the record is still written -- all zeros)
    hipLaunchKernelGGL(masked_nll_finalize_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, part, blocks,
                       reinterpret_cast<unsigned long long *>(stats));
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
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
