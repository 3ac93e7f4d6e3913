// pgcn_loss_multilabel.hip -- masked binary cross entropy with logits and the micro-F1 counts of multi-label node
// classification, forward and backward, for gfx950 (the multi-label sibling of the masked kernels of pgcn_loss.hip).
//
//   loss_ij = y_ij ? softplus(-x_ij) : softplus(x_ij),   softplus(t) = max(t, 0) + log1p(exp(-|t|))
//   dx_ij   = g * (sigmoid(x_ij) - y_ij)  on train rows, 0 elsewhere
//
// Every row carries a split code (0 in no set, 1 train, 2 val, 3 test) and ceil(C / 32) label words in the sign-mask layout
// (bit b of word w = label 32 w + b).  ONE pass over the logits leaves, per set, the sum of the element losses and the numbers
// of true positives, false positives and false negatives of the prediction x > 0: the training loss and the three micro-F1
// of a step without logits[mask] (a host synchronisation), without a threshold and three comparisons per set.  Rows in no set
// are skipped: neither their logits nor their label words are read.  A block owns 64 consecutive rows and writes one partial
// record; a second, one-block launch adds the records in block order -- no floating-point atomics, two calls give the same bits.
//
// Lanes per row as in pgcn_loss.hip: 16 lanes own a row (float4 chunks c = sub, sub + 16, ...; four rows per wave) when
// C % 4 == 0 and the rows are 16-byte aligned -- for EVERY such C up to 1024: a chunk never straddles a label word, and nothing
// needs C % 32 == 0 -- and a wave per row (lane j takes columns j, j + 64, ...) otherwise.  The label words of a row are loaded
// ONCE by the lanes that own the row (lane l takes word l, and word l + 16 in the 16-lane scheme) and handed round by
// ds_bpermute: 4 C + C / 8 + 1 bytes per row of a set forward, 1 byte for a row in none.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxColumns = 1024;
constexpr int kBlockRows = 64;           // rows per block of the forward: one partial record per 64 rows
constexpr int kStatWords = 20;           // pgcn_masked_bce_stats: double loss_sum[4], int64 tp[4], fp[4], fn[4], rows[4]
constexpr int kCounts = 13;              // tp[1..3], fp[1..3], fn[1..3], rows[0..3]

// one element: its loss and its part of the counts (tp in bits 0.., fp in bits 16.. of `tpfp`: at most 1024 each per row)
__device__ __forceinline__ void bce_element(float x, bool y, float &loss, int &tpfp, int &fn) {
    const float t = y ? -x : x;
    // fmaxf drops a NaN, expf keeps it: NaN logits give a NaN loss; +-inf give 0 or +inf, never inf - inf
    loss += fmaxf(t, 0.f) + log1pf(expf(-fabsf(x)));
    const bool pred = x > 0.f;           // x == 0 and NaN predict negative
    tpfp += pred ? (y ? 1 : 0x10000) : 0;
    fn += (!pred && y) ? 1 : 0;
}

// sigmoid with exactly 1 / 0 at +-inf: 1 / (1 + exp(-x)) for x >= 0, e / (1 + e) with e = exp(x) below
__device__ __forceinline__ float sigmoidf(float x) {
    const float e = expf(-fabsf(x));
    const float r = 1.f / (1.f + e);
    return x >= 0.f ? r : e * r;         // (a NaN takes the second branch and stays NaN)
}

// what one lane has seen of the rows it leads (slot 0 = rows in no set: counted, nothing else)
struct BceAcc {
    double loss[3];
    int tp[3], fp[3], fn[3];
    int rows[4];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            loss[s] = 0.0;
            tp[s] = fp[s] = fn[s] = 0;
        }
        rows[0] = rows[1] = rows[2] = rows[3] = 0;
    }
    // selects, not products: a NaN row loss reaches its own set only
    __device__ __forceinline__ void add(int k, float row_loss, int tpfp, int f) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const bool mine = k == s + 1;
            loss[s] += mine ? (double)row_loss : 0.0;
            tp[s] += mine ? (tpfp & 0xffff) : 0;
            fp[s] += mine ? (tpfp >> 16) : 0;
            fn[s] += mine ? f : 0;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) rows[s] += (k == s) ? 1 : 0;
    }
};

// butterfly over the wave, then the block's four waves in order: one record per block, fixed order
__device__ __forceinline__ void bce_block_store(BceAcc &acc, unsigned long long *__restrict__ part) {
    __shared__ double s_loss[kThreads / 64][3];
    __shared__ int s_cnt[kThreads / 64][kCounts];
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            acc.loss[s] += __shfl_xor(acc.loss[s], o, 64);
            acc.tp[s] += __shfl_xor(acc.tp[s], o, 64);
            acc.fp[s] += __shfl_xor(acc.fp[s], o, 64);
            acc.fn[s] += __shfl_xor(acc.fn[s], o, 64);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc.rows[s] += __shfl_xor(acc.rows[s], o, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            s_loss[w][s] = acc.loss[s];
            s_cnt[w][s] = acc.tp[s];
            s_cnt[w][3 + s] = acc.fp[s];
            s_cnt[w][6 + s] = acc.fn[s];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) s_cnt[w][9 + s] = acc.rows[s];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *pl = reinterpret_cast<double *>(part + (size_t)blockIdx.x * kStatWords);
        long long *pc = reinterpret_cast<long long *>(part + (size_t)blockIdx.x * kStatWords) + 4;
        pl[0] = 0.0;
        for (int s = 0; s < 3; ++s) {
            double a = s_loss[0][s];
            for (int v = 1; v < kThreads / 64; ++v) a += s_loss[v][s];
            pl[1 + s] = a;
        }
        for (int q = 0; q < 3; ++q) {                     // tp, fp, fn: slot 0 is zero
            pc[4 * q] = 0;
            for (int s = 0; s < 3; ++s) {
                long long c = s_cnt[0][3 * q + s];
                for (int v = 1; v < kThreads / 64; ++v) c += s_cnt[v][3 * q + s];
                pc[4 * q + 1 + s] = c;
            }
        }
        for (int s = 0; s < 4; ++s) {
            long long c = s_cnt[0][9 + s];
            for (int v = 1; v < kThreads / 64; ++v) c += s_cnt[v][9 + s];
            pc[12 + s] = c;
        }
    }
}

__device__ __forceinline__ int split_code(const uint8_t *__restrict__ split, int64_t i) {
    const int s = split[i];
    return s <= 3 ? s : 0;
}

// every other width: a wave owns a row (lane j takes columns j, j + 64, ...), 4 rows per step, 16 steps per block
__global__ __launch_bounds__(kThreads) void masked_bce_kernel(const float *__restrict__ X, int64_t ldx,
                                                              const uint32_t *__restrict__ labels,
                                                              const uint8_t *__restrict__ split, int64_t nrows, int32_t C,
                                                              unsigned long long *__restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = (C + 31) >> 5, nq = (C + 63) >> 6;
    BceAcc acc;
    acc.clear();
    for (int it = 0; it < kBlockRows / 4; ++it) {
        const int64_t i = (int64_t)blockIdx.x * kBlockRows + it * 4 + wave;
        if (i >= nrows) break;                            // (wave-uniform)
        const int k = split_code(split, i);               // (wave-uniform: one row per wave)
        float loss = 0.f;
        int tpfp = 0, fn = 0;
        if (k != 0) {
            const float *x = X + i * ldx;
            const uint32_t mine = lane < nw ? labels[i * nw + lane] : 0u;        // nw <= 32: lane l holds word l
            for (int q = 0; q < nq; ++q) {
                const int j = lane + 64 * q;
                const uint32_t word = __shfl(mine, (lane >> 5) + 2 * q, 64);     // word j / 32 (every lane takes part)
                if (j < C) bce_element(x[j], (word >> (lane & 31)) & 1u, loss, tpfp, fn);
            }
            for (int o = 32; o > 0; o >>= 1) {
                loss += __shfl_xor(loss, o, 64);
                tpfp += __shfl_xor(tpfp, o, 64);
                fn += __shfl_xor(fn, o, 64);
            }
        }
        if (lane == 0) acc.add(k, loss, tpfp, fn);
    }
    bce_block_store(acc, part);
}

// C % 4 == 0, 16-byte aligned rows: 16 lanes own a row (float4 chunks c = sub, sub + 16, ...), 16 rows per step, 4 steps per
// block.  Chunk c holds columns 4 c .. 4 c + 3 = bits 4 (c & 7) .. of word c / 8; lane `sub` of the group holds words sub and
// sub + 16 of its row.
__global__ __launch_bounds__(kThreads) void masked_bce_v4_kernel(const float *__restrict__ X, int64_t ldx,
                                                                 const uint32_t *__restrict__ labels,
                                                                 const uint8_t *__restrict__ split, int64_t nrows, int32_t C,
                                                                 unsigned long long *__restrict__ part) {
    const int lane = threadIdx.x & 63, sub = lane & 15, base = lane & 48;
    const int nch = C >> 2, nw = (C + 31) >> 5, nq = (nch + 15) >> 4;
    BceAcc acc;
    acc.clear();
#pragma unroll 1
    for (int it = 0; it < kBlockRows / 16; ++it) {
        const int64_t i = (int64_t)blockIdx.x * kBlockRows + it * 16 + (threadIdx.x >> 6) * 4 + (lane >> 4);
        const bool act = i < nrows;
        const int k = act ? split_code(split, i) : 0;
        const bool live = k != 0;                         // (uniform over the 16 lanes of a row)
        const float4 *x4 = reinterpret_cast<const float4 *>(X + (live ? i : 0) * ldx);
        const uint32_t *lw = labels + (live ? i : 0) * nw;
        const uint32_t w0 = (live && sub < nw) ? lw[sub] : 0u;
        const uint32_t w1 = (live && sub + 16 < nw) ? lw[sub + 16] : 0u;
        float loss = 0.f;
        int tpfp = 0, fn = 0;
        for (int q = 0; q < nq; ++q) {                    // (nq is the same for every lane: the shuffles see whole waves)
            const int c = sub + 16 * q;
            const int wi = c >> 3;                        // = (sub >> 3) + 2 q: below 16 exactly when q < 8
            const uint32_t word = __shfl(q < 8 ? w0 : w1, base + (wi & 15), 64);
            if (live && c < nch) {
                const float4 v = x4[c];
                const uint32_t b = word >> (4 * (c & 7));
                bce_element(v.x, b & 1u, loss, tpfp, fn);
                bce_element(v.y, b & 2u, loss, tpfp, fn);
                bce_element(v.z, b & 4u, loss, tpfp, fn);
                bce_element(v.w, b & 8u, loss, tpfp, fn);
            }
        }
        for (int o = 8; o > 0; o >>= 1) {
            loss += __shfl_xor(loss, o, 64);
            tpfp += __shfl_xor(tpfp, o, 64);
            fn += __shfl_xor(fn, o, 64);
        }
        if (act && sub == 0) acc.add(k, loss, tpfp, fn);
    }
    bce_block_store(acc, part);
}

// one block: thread t adds records t, t + 256, ... in that order, then the same butterfly / wave order as above
__global__ __launch_bounds__(kThreads) void masked_bce_finalize_kernel(const unsigned long long *__restrict__ part, int64_t nblocks,
                                                                       unsigned long long *__restrict__ stats) {
    __shared__ double s_loss[kThreads / 64][3];
    __shared__ long long s_cnt[kThreads / 64][kCounts];
    double loss[3] = {0.0, 0.0, 0.0};
    long long cnt[kCounts];
#pragma unroll
    for (int s = 0; s < kCounts; ++s) cnt[s] = 0;
    for (int64_t b = threadIdx.x; b < nblocks; b += kThreads) {
        const double *pl = reinterpret_cast<const double *>(part + b * kStatWords);
        const long long *pc = reinterpret_cast<const long long *>(part + b * kStatWords) + 4;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            loss[s] += pl[1 + s];
            cnt[s] += pc[1 + s];
            cnt[3 + s] += pc[5 + s];
            cnt[6 + s] += pc[9 + s];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) cnt[9 + s] += pc[12 + s];
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int s = 0; s < 3; ++s) loss[s] += __shfl_xor(loss[s], o, 64);
#pragma unroll
        for (int s = 0; s < kCounts; ++s) cnt[s] += __shfl_xor(cnt[s], o, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int s = 0; s < 3; ++s) s_loss[w][s] = loss[s];
#pragma unroll
        for (int s = 0; s < kCounts; ++s) s_cnt[w][s] = cnt[s];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *ol = reinterpret_cast<double *>(stats);
        long long *oc = reinterpret_cast<long long *>(stats) + 4;
        ol[0] = 0.0;
        for (int s = 0; s < 3; ++s) {
            double a = s_loss[0][s];
            for (int v = 1; v < kThreads / 64; ++v) a += s_loss[v][s];
            ol[1 + s] = a;
        }
        for (int q = 0; q < 3; ++q) {
            oc[4 * q] = 0;
            for (int s = 0; s < 3; ++s) {
                long long c = s_cnt[0][3 * q + s];
                for (int v = 1; v < kThreads / 64; ++v) c += s_cnt[v][3 * q + s];
                oc[4 * q + 1 + s] = c;
            }
        }
        for (int s = 0; s < 4; ++s) {
            long long c = s_cnt[0][9 + s];
            for (int v = 1; v < kThreads / 64; ++v) c += s_cnt[v][9 + s];
            oc[12 + s] = c;
        }
    }
}

__global__ __launch_bounds__(kThreads) void masked_bce_backward_kernel(const float *__restrict__ X, int64_t ldx,
                                                                       const uint32_t *__restrict__ labels,
                                                                       const uint8_t *__restrict__ split,
                                                                       const float *__restrict__ gscale, float scale,
                                                                       int64_t nrows, int32_t C, float *__restrict__ dX,
                                                                       int64_t lddx) {
    const int64_t i = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= nrows) return;                               // (wave-uniform)
    float *dx = dX + i * lddx;
    if (split[i] != 1) {                                  // not a train row: exact zeros, its logits and labels are not read
        for (int j = lane; j < C; j += 64) dx[j] = 0.f;
        return;
    }
    const float g = (gscale ? gscale[0] : 1.f) * scale;
    const float *x = X + i * ldx;
    const int nw = (C + 31) >> 5, nq = (C + 63) >> 6;
    const uint32_t mine = lane < nw ? labels[i * nw + lane] : 0u;
    for (int q = 0; q < nq; ++q) {
        const int j = lane + 64 * q;
        const uint32_t word = __shfl(mine, (lane >> 5) + 2 * q, 64);
        if (j < C) dx[j] = g * (sigmoidf(x[j]) - (float)((word >> (lane & 31)) & 1u));
    }
}

__global__ __launch_bounds__(kThreads) void masked_bce_backward_v4_kernel(const float *__restrict__ X, int64_t ldx,
                                                                          const uint32_t *__restrict__ labels,
                                                                          const uint8_t *__restrict__ split,
                                                                          const float *__restrict__ gscale, float scale,
                                                                          int64_t nrows, int32_t C, float *__restrict__ dX,
                                                                          int64_t lddx) {
    const int lane = threadIdx.x & 63, sub = lane & 15, base = lane & 48;
    const int64_t i = ((int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) * 4 + (lane >> 4);
    if (i >= nrows) return;                               // (uniform over the 16 lanes of a row, like every branch below)
    float4 *d4 = reinterpret_cast<float4 *>(dX + i * lddx);
    const int nch = C >> 2;
    if (split[i] != 1) {
        for (int c = sub; c < nch; c += 16) d4[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float g = (gscale ? gscale[0] : 1.f) * scale;
    const float4 *x4 = reinterpret_cast<const float4 *>(X + i * ldx);
    const int nw = (C + 31) >> 5, nq = (nch + 15) >> 4;
    const uint32_t *lw = labels + i * nw;
    const uint32_t w0 = sub < nw ? lw[sub] : 0u;
    const uint32_t w1 = sub + 16 < nw ? lw[sub + 16] : 0u;
    for (int q = 0; q < nq; ++q) {
        const int c = sub + 16 * q;
        const uint32_t word = __shfl(q < 8 ? w0 : w1, base + ((c >> 3) & 15), 64);       // (read from the row's own 16 lanes)
        if (c < nch) {
            const float4 v = x4[c];
            const uint32_t b = word >> (4 * (c & 7));
            d4[c] = make_float4(g * (sigmoidf(v.x) - (float)(b & 1u)), g * (sigmoidf(v.y) - (float)((b >> 1) & 1u)),
                                g * (sigmoidf(v.z) - (float)((b >> 2) & 1u)), g * (sigmoidf(v.w) - (float)((b >> 3) & 1u)));
        }
    }
}

}  // namespace

extern "C" int64_t pgcn_masked_bce_ws_bytes(int64_t nrows) {
    const int64_t blocks = nrows > 0 ? (nrows + kBlockRows - 1) / kBlockRows : 1;
    return blocks * kStatWords * (int64_t)sizeof(unsigned long long);
}

extern "C" int pgcn_masked_bce_f32(const float *X, int64_t ldx, const uint32_t *labels, const uint8_t *split, int64_t nrows,
                                   int32_t C, pgcn_masked_bce_stats *stats, void *ws, int64_t ws_bytes, pgcn_stream_t stream) {
    static_assert(sizeof(pgcn_masked_bce_stats) == kStatWords * sizeof(unsigned long long), "record layout");
    if (nrows < 0 || C <= 0 || ldx < C) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_f32: bad sizes");
    if (C > kMaxColumns) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_masked_bce_f32: more than 1024 columns");
    if (!stats || (uintptr_t)stats % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_f32: stats must be 8-byte aligned");
    const int64_t blocks = (nrows + kBlockRows - 1) / kBlockRows;
    if (blocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_f32: too many rows");
    unsigned long long *part = static_cast<unsigned long long *>(ws);
    if (nrows > 0) {
        if (!X || !labels || !split) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_f32: null pointer");
        if ((uintptr_t)labels % 4 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_f32: labels must be 4-byte aligned");
        if (!ws || (uintptr_t)ws % 8 != 0 || ws_bytes < pgcn_masked_bce_ws_bytes(nrows))
            return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_f32: work-space too small or not 8-byte aligned");
        const dim3 grid((unsigned)blocks), block(kThreads);
        if (C % 4 == 0 && ldx % 4 == 0 && (uintptr_t)X % 16 == 0)
            hipLaunchKernelGGL(masked_bce_v4_kernel, grid, block, 0, (hipStream_t)stream, X, ldx, labels, split, nrows, C, part);
        else
            hipLaunchKernelGGL(masked_bce_kernel, grid, block, 0, (hipStream_t)stream, X, ldx, labels, split, nrows, C, part);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    // (no rows: the record is still written -- all zeros)
    hipLaunchKernelGGL(masked_bce_finalize_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, part, blocks,
                       reinterpret_cast<unsigned long long *>(stats));
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_masked_bce_backward_f32(const float *X, int64_t ldx, const uint32_t *labels, const uint8_t *split,
                                            const float *gscale_dev, float scale, int64_t nrows, int32_t C, float *dX,
                                            int64_t lddx, pgcn_stream_t stream) {
    if (nrows < 0 || C <= 0 || ldx < C || lddx < C) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_backward_f32: bad sizes");
    if (C > kMaxColumns) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_masked_bce_backward_f32: more than 1024 columns");
    if (nrows == 0) return PGCN_OK;
    if (!X || !labels || !split || !dX) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_backward_f32: null pointer");
    if ((uintptr_t)labels % 4 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_backward_f32: labels must be 4-byte aligned");
    if (C % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)dX % 16 == 0) {
        const int64_t g4 = (nrows + 15) / 16;
        if (g4 > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_backward_f32: too many rows");
        hipLaunchKernelGGL(masked_bce_backward_v4_kernel, dim3((unsigned)g4), dim3(kThreads), 0, (hipStream_t)stream, X, ldx,
                           labels, split, gscale_dev, scale, nrows, C, dX, lddx);
        PGCN_HIP_CHECK(hipGetLastError());
        return PGCN_OK;
    }
    const int64_t grid = (nrows + 3) / 4;
    if (grid > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_backward_f32: too many rows");
    hipLaunchKernelGGL(masked_bce_backward_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, X, ldx, labels,
                       split, gscale_dev, scale, nrows, C, dX, lddx);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}
