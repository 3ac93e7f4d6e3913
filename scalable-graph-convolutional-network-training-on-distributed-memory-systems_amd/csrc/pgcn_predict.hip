// pgcn_predict.hip -- one pass from the logits of a block of vertices to what a user stores, for gfx950 (checkpoint.py: write_predictions;
// include/pgcn_hip.h has the contract).
//
//   task 0 (one class per row)   m_i = max_j x_ij;  cls_i = the lowest j with x_ij == m_i  (the rule of pgcn_masked_nll_f32: fmaxf drops a
//                                NaN, a NaN equals nothing; no such j, a row of NaN only: -1, which no label equals)
//                                e_ij = expf(x_ij - m_i);  s_i = sum_j e_ij;  conf_i = 1 / s_i;  prob_ij = e_ij / s_i
//   task 1 (multi-label)         bit (i, j) = x_ij > 0  (the rule of pgcn_masked_bce_f32; a NaN is not > 0);  prob_ij = 1 / (1 + expf(-x_ij))
//
// Row-local, no atomics, no work-space: a row's outputs are a function of that row alone -- not of its index, the block that met it or
// nrows.  The layout of pgcn_rowband.h, one row per thread in flight; csrc/build.sh compiles this file with -ffp-contract=off, and
// nothing in it could be fused anyway (differences, sums, quotients), so the float4 path and the guarded scalar path leave the same bits.
//
// Row maximum, row sum (fp32) and the arg-max: a thread folds its quad in a fixed order, columns at and beyond C as -inf / 0 / no column;
// then an xor butterfly over the row's aligned group of TPR lanes (TPR <= 64: inside one wave; the operations commute, so every lane
// ends with the same value -- a maximum of +0 and -0 may differ in sign between lanes, which neither the comparison nor expf(x - m)
// sees); TPR = 128 or 256: the butterfly over the whole wave, lane 0 of each wave leaves its partial in LDS, every thread folds its row's
// 2 or 4 partials as (p0, p1) [, (p2, p3)].  EVERY thread of a block walks every iteration (rows beyond the band and columns beyond C
// compute on neutral values and store nothing): the shuffles and the barriers are never divergent.  The label bits: 8 neighbouring
// threads hold one 32-bit word, or-ed by three shuffles, the first of the 8 stores it (the layout of nodedata.pack_label_words).
// Raw pointers + a stream, no allocation, no synchronisation: graph-capturable.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"
#include "pgcn_rowband.h"

namespace {

constexpr int kWaves = kThreads / 64;
constexpr int kNoColumn = 0x7fffffff;

struct MaxOp {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
struct SumOp {
    __device__ __forceinline__ float operator()(float a, float b) const { return a + b; }
};
struct MinOp {
    __device__ __forceinline__ int operator()(int a, int b) const { return a < b ? a : b; }
};

// v <- op over the tpr threads of this thread's row, the same value in every one of them.  CROSS (tpr = 128 or 256): `sm` holds
// 2 x kWaves words, `phase` picks the half -- successive calls alternate, so that ONE barrier per call is enough (a wave that runs
// ahead writes the other half; the half it will write after that was last read before the barrier between).
template <bool CROSS, class T, class Op>
__device__ __forceinline__ T row_fold(T v, Op op, int tpr, T *sm, int phase, int tid) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        if (m < tpr) v = op(v, __shfl_xor(v, m, 64));          // (uniform over the block)
    }
    if constexpr (CROSS) {
        const int wave = tid >> 6;
        T *s = sm + (phase & 1) * kWaves;
        if ((tid & 63) == 0) s[wave] = v;
        __syncthreads();
        if (tpr == kThreads) {
            v = op(op(s[0], s[1]), op(s[2], s[3]));
        } else {
            const int w0 = wave & ~1;
            v = op(s[w0], s[w0 + 1]);
        }
    }
    return v;
}

template <bool VEC, bool CROSS>
__global__ __launch_bounds__(kThreads) void classes_kernel(const float *__restrict__ X, int64_t ldx, int64_t nrows, int C, int log2_tpr,
                                                           int64_t *__restrict__ cls, float *__restrict__ conf, float *__restrict__ prob,
                                                           int64_t ldp) {
#pragma clang fp contract(off)
    __shared__ float smf[2 * 2 * kWaves];     // the maxima (phases 0 / 1 of the first half), the sums (the second half)
    __shared__ int smi[2 * kWaves];
    const int tid = threadIdx.x;
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kApplyRows, nrows);
    const bool active = c0 < C;
    int phase = 0;
    for (int64_t base = r0; base < rend; base += ngroups, ++phase) {          // (uniform over the block)
        const int64_t rr = base + rg;
        const bool ok = rr < rend && active;
        Quad q;
        if (ok) q = load_quad<VEC>(X + rr * ldx, c0, C);
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!(ok && c0 + j < C)) q.v[j] = -INFINITY;
            m = fmaxf(m, q.v[j]);
        }
        m = row_fold<CROSS>(m, MaxOp(), tpr, smf, phase, tid);
        Quad e;
        int best = kNoColumn;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            const bool col = ok && c0 + j < C;
            e.v[j] = col ? expf(q.v[j] - m) : 0.f;
            if (col && q.v[j] == m) best = c0 + j;
        }
        float s = ((e.v[0] + e.v[1]) + e.v[2]) + e.v[3];
        s = row_fold<CROSS>(s, SumOp(), tpr, smf + 2 * kWaves, phase, tid);
        best = row_fold<CROSS>(best, MinOp(), tpr, smi, phase, tid);
        if (ok) {
            if (u == 0) {
                if (cls) cls[rr] = best == kNoColumn ? (int64_t)-1 : (int64_t)best;
                if (conf) conf[rr] = 1.0f / s;
            }
            if (prob) {
#pragma unroll
                for (int j = 0; j < 4; ++j) e.v[j] = e.v[j] / s;
                store_quad<VEC>(prob + rr * ldp, c0, C, e);
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void labels_kernel(const float *__restrict__ X, int64_t ldx, int64_t nrows, int C, int log2_tpr,
                                                          uint32_t *__restrict__ bits, float *__restrict__ prob, int64_t ldp) {
#pragma clang fp contract(off)
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kApplyRows, nrows);
    const bool active = c0 < C;
    const int mw = (C + 31) >> 5;
    for (int64_t base = r0; base < rend; base += ngroups) {                   // (uniform over the block)
        const int64_t rr = base + rg;
        const bool ok = rr < rend && active;
        Quad q = Quad{{0.f, 0.f, 0.f, 0.f}};
        if (ok) q = load_quad<VEC>(X + rr * ldx, c0, C);
        if (bits) {                                                           // (uniform: every lane takes the shuffles)
            uint32_t b = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ok && c0 + j < C && q.v[j] > 0.f) b |= 1u << j;
            uint32_t word = b << (4 * (u & 7));                               // 8 neighbouring threads hold one word
#pragma unroll
            for (int m = 1; m < 8; m <<= 1)
                if (m < tpr) word |= (uint32_t)__shfl_xor((int)word, m, 64);
            if (ok && (u & 7) == 0) bits[rr * mw + (u >> 3)] = word;
        }
        if (prob && ok) {
            Quad p;
#pragma unroll
            for (int j = 0; j < 4; ++j) p.v[j] = 1.0f / (1.0f + expf(-q.v[j]));
            store_quad<VEC>(prob + rr * ldp, c0, C, p);
        }
    }
}

}  // namespace

extern "C" int pgcn_predict_f32(const float *X, int64_t ldx, int64_t nrows, int32_t C, int32_t task, int64_t *cls, float *conf,
                                uint32_t *bits, float *prob, int64_t ldp, pgcn_stream_t stream) {
    if (nrows < 0 || C < 1 || C > kMaxF) return pgcn_set_error(PGCN_EINVAL, "pgcn_predict_f32: nrows < 0, C < 1 or C > 1024");
    if (ldx < C || (prob && ldp < C)) return pgcn_set_error(PGCN_EINVAL, "pgcn_predict_f32: a leading dimension is below C");
    if (task != 0 && task != 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_predict_f32: task must be 0 (one class per row) or 1 (multi-label)");
    if (nrows > 0 && !X) return pgcn_set_error(PGCN_EINVAL, "pgcn_predict_f32: null pointer");
    if ((cls && (uintptr_t)cls % 8 != 0) || (uintptr_t)X % 4 != 0 || (conf && (uintptr_t)conf % 4 != 0) ||
        (bits && (uintptr_t)bits % 4 != 0) || (prob && (uintptr_t)prob % 4 != 0))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_predict_f32: a misaligned pointer (cls: 8 bytes, the others: 4)");
    const int64_t nblocks = apply_blocks(nrows);
    if (nblocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_predict_f32: too many rows");
    if (nrows == 0) return PGCN_OK;
    const int l2 = log2_threads_per_row(C);
    const bool vec = C % 4 == 0 && rows16(ldx) && aligned16(X) && (!prob || (rows16(ldp) && aligned16(prob)));
    hipStream_t s = (hipStream_t)stream;
    if (task == 0) {
        if (!cls && !conf && !prob) return PGCN_OK;
        const bool cross = l2 > 6;
        launch(cross ? (vec ? classes_kernel<true, true> : classes_kernel<false, true>)
                     : (vec ? classes_kernel<true, false> : classes_kernel<false, false>),
               nblocks, s, X, ldx, nrows, C, l2, cls, conf, prob, ldp);
    } else {
        if (!bits && !prob) return PGCN_OK;
        launch(vec ? labels_kernel<true> : labels_kernel<false>, nblocks, s, X, ldx, nrows, C, l2, bits, prob, ldp);
    }
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}
