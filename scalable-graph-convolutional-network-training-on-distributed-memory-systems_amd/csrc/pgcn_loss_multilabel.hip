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
// record; a second, one-block launch adds the records (pgcn_setrecord.h: the record, the fixed order of its sums and its promise).
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
#include "pgcn_setrecord.h"

namespace {

constexpr int kMaxColumns = 1024;
using BceRecord = SetRecord<3>;          // pgcn_masked_bce_stats: double loss_sum[4], int64 tp[4], fp[4], fn[4], rows[4]
static_assert(sizeof(pgcn_masked_bce_stats) == BceRecord::kWords * sizeof(unsigned long long), "record layout");

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

// a row of set k to its leader's record: tp, fp unpacked, fn
__device__ __forceinline__ void bce_row(BceRecord &acc, int k, float loss, int tpfp, int fn) {
    const int c[3] = {tpfp & 0xffff, tpfp >> 16, fn};
    acc.add(k, loss, c);
}

// every other width: a wave owns a row (lane j takes columns j, j + 64, ...), 4 rows per step, 16 steps per block
__global__ __launch_bounds__(kThreads) void masked_bce_kernel(const float *__restrict__ X, int64_t ldx,
                                                              const uint32_t *__restrict__ labels,
                                                              const uint8_t *__restrict__ split, int64_t nrows, int32_t C,
                                                              unsigned long long *__restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = (C + 31) >> 5, nq = (C + 63) >> 6;
    BceRecord acc;
    acc.clear();
    for (int it = 0; it < kSetRows / 4; ++it) {
        const int64_t i = (int64_t)blockIdx.x * kSetRows + it * 4 + wave;
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
        if (lane == 0) bce_row(acc, k, loss, tpfp, fn);
    }
    acc.block_store(part);
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
    BceRecord acc;
    acc.clear();
#pragma unroll 1
    for (int it = 0; it < kSetRows / 16; ++it) {
        const int64_t i = (int64_t)blockIdx.x * kSetRows + it * 16 + (threadIdx.x >> 6) * 4 + (lane >> 4);
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
        if (act && sub == 0) bce_row(acc, k, loss, tpfp, fn);
    }
    acc.block_store(part);
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

extern "C" int64_t pgcn_masked_bce_ws_bytes(int64_t nrows) { return set_ws_bytes<3>(nrows); }

extern "C" int pgcn_masked_bce_f32(const float *X, int64_t ldx, const uint32_t *labels, const uint8_t *split, int64_t nrows,
                                   int32_t C, pgcn_masked_bce_stats *stats, void *ws, int64_t ws_bytes, pgcn_stream_t stream) {
    if (nrows < 0 || C <= 0 || ldx < C) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_f32: bad sizes");
    if (C > kMaxColumns) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_masked_bce_f32: more than 1024 columns");
    int64_t blocks;
    if (int rc = set_check_record("pgcn_masked_bce_f32", stats, nrows, &blocks)) return rc;
    unsigned long long *part = static_cast<unsigned long long *>(ws);
    if (nrows > 0) {
        if (!X || !labels || !split) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_f32: null pointer");
        if ((uintptr_t)labels % 4 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_masked_bce_f32: labels must be 4-byte aligned");
        if (int rc = set_check_ws<3>("pgcn_masked_bce_f32", ws, ws_bytes, nrows)) return rc;
        const dim3 grid((unsigned)blocks), block(kThreads);
        if (C % 4 == 0 && ldx % 4 == 0 && (uintptr_t)X % 16 == 0)
            hipLaunchKernelGGL(masked_bce_v4_kernel, grid, block, 0, (hipStream_t)stream, X, ldx, labels, split, nrows, C, part);
        else
            hipLaunchKernelGGL(masked_bce_kernel, grid, block, 0, (hipStream_t)stream, X, ldx, labels, split, nrows, C, part);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    return set_finalize<3>(ws, blocks, stats, stream);
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
