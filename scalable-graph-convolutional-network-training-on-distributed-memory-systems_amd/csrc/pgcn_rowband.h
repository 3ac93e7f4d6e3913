// pgcn_rowband.h -- the layout, the dropout pieces and the deterministic column sums that the row-band layer kernels share
// (pgcn_norm.hip, pgcn_combine.hip, pgcn_layernorm.hip, pgcn_gat_tail.hip; pgcn_predict.hip takes the layout alone).  Header-only, everything in an anonymous namespace: each
// translation unit keeps its own copy under its own compile flags.  Nothing in here depends on -ffp-contract: the floating-point
// work is additions of doubles, nothing a contraction could fuse; the element arithmetic stays in the including file.
//
// Layout, the same in every kernel: 256 threads; a thread owns FOUR consecutive columns (one float4), TPR = the power of two
// >= ceil(f / 4) threads span a row, 256 / TPR row groups walk a band of consecutive rows (kApplyRows for an element-wise pass,
// kSumRows where column sums are formed), a few rows per thread in flight (the kernel's own choice).  What belongs to a column (a
// bias, gamma, the column's share of the dropout hash) is loaded or computed once per thread, before the row loop.  f <= 1024 is
// what 256 threads x 4 columns cover.  When f % 4 == 0 and every base and leading dimension keeps the rows 16-byte aligned the four
// columns move as one float4; otherwise the SAME thread moves them as four guarded scalars -- the same thread does the same
// arithmetic in the same order, so both paths leave the same bits.  Row addresses are 64-bit.
//
// Column sums: a block owns kSumRows consecutive rows; its threads add in double registers, the row groups are folded through LDS
// by a fixed tree (fold_row_groups) and the block writes ONE partial record of 1 or 2 x f doubles to the work-space
// (write_partial).  The second launch gives each block 32 of the outputs: 8 groups of threads add the records b = group,
// group + 8, ... in that order, a fixed tree folds the 8 (final_sum) -- no floating-point atomics, the same input gives the same
// bits; at the Reddit shape (232 965 x 128) that is 456 bands.  NaN and inf stay in their own column: no thread touches two
// columns' sums.  Every barrier in here is reached by the whole block.
#ifndef PGCN_ROWBAND_H
#define PGCN_ROWBAND_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PG_DROPOUT_FN __host__ __device__ __forceinline__
#include "../gemm/pgcn_dropout.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSumRows = 512;      // rows of a band of the column-sum kernels (kernels.ROWBAND_SUM_ROWS restates it)
constexpr int kApplyRows = 128;    // rows of a band of the element-wise kernels
constexpr int kFinalCols = 32;     // outputs of a block of the second level
constexpr int kFinalGroups = kThreads / kFinalCols;
constexpr int kMaxF = 1024;        // (kernels.ROWBAND_MAX_F restates it)

struct Quad {
    float v[4];
};

// (no __restrict__ on the rows: an output may be an input itself; a thread reads its own elements before it writes them)
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

// a column's constant (0 beyond the last column: such a lane computes on zeros and stores nothing)
__device__ __forceinline__ Quad load_cols(const float *__restrict__ p, int c0, int f) {
    Quad q;
#pragma unroll
    for (int j = 0; j < 4; ++j) q.v[j] = c0 + j < f ? p[c0 + j] : 0.f;
    return q;
}

// A thread's place: tpr threads span a row, this one is column quad u of row group rg (of ngroups), first column c0; its block's
// rows are r0 .. rend - 1.
struct Band {
    int tpr, u, rg, ngroups, c0;
    int64_t r0, rend;
};

__device__ __forceinline__ Band band_of(int log2_tpr, int band_rows, int64_t nrows) {
    const int tid = threadIdx.x, tpr = 1 << log2_tpr, u = tid & (tpr - 1);
    const int64_t r0 = (int64_t)blockIdx.x * band_rows;
    return Band{tpr, u, tid >> log2_tpr, kThreads >> log2_tpr, 4 * u, r0, r0 + band_rows < nrows ? r0 + band_rows : nrows};
}

// ---- dropout: the keep function of gemm/pgcn_dropout.h, the column's share once per thread, the row's once per row ----
struct DropArgs {
    const int64_t *row_ids;    // NULL: the row index is the global id
    const int64_t *step;       // NULL: no dropout
    uint64_t seed;
    uint32_t layer, thr;
    float scale, inv_scale;
};

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

// (The device pieces take DropArgs' fields one by one: through a reference to a kernel's by-value argument the compiler would copy
// the whole struct first, and the kernels would no longer compile to what they were before these pieces were shared.)
struct DropCols {
    bool on;
    uint64_t key;
    uint32_t col[4];
};

// once per thread, before the row loop
__device__ __forceinline__ DropCols drop_cols(const int64_t *step, uint64_t seed, uint32_t layer, int c0, bool enabled = true) {
    DropCols c = {enabled && step != nullptr, 0, {0, 0, 0, 0}};
    if (c.on) {
        c.key = dropout_key(seed, (uint64_t)step[0], layer);
#pragma unroll
        for (int j = 0; j < 4; ++j) c.col[j] = dropout_col(c.key, (uint32_t)(c0 + j));
    }
    return c;
}

struct DropRow {
    uint32_t term, hi;
};

// once per row, where c.on
__device__ __forceinline__ DropRow drop_row(const int64_t *row_ids, const DropCols &c, int64_t row) {
    const uint64_t grow = row_ids ? (uint64_t)row_ids[row] : (uint64_t)row;
    return DropRow{dropout_row(c.key, grow), (uint32_t)(grow >> 32)};
}

// whether the element of the thread's column j survives
__device__ __forceinline__ bool drop_keep(const DropCols &c, const DropRow &r, int j, uint32_t thr) {
    return dropout_u(c.col[j], r.term, r.hi) >= thr;
}

// ---- column sums ----
// Folds the 256 / TPR row groups of `acc` (N = 4 or 8 doubles per thread) through `sm` (N x 256 doubles of LDS), k-major so that
// neighbouring threads touch neighbouring doubles; on return the threads of row group 0 hold the band's sums.
template <int N>
__device__ __forceinline__ void fold_row_groups(double (&acc)[N], double *sm, int log2_tpr) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) sm[k * kThreads + tid] = acc[k];
    for (int s = (kThreads >> log2_tpr) >> 1; s >= 1; s >>= 1) {
        __syncthreads();
        if ((tid >> log2_tpr) < s) {
#pragma unroll
            for (int k = 0; k < N; ++k) sm[k * kThreads + tid] += sm[k * kThreads + tid + (s << log2_tpr)];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = sm[k * kThreads + tid];
}

// the band's record: f doubles (N = 4) or [2][f] (N = 8: acc[4 ..] are the second sums)
template <int N>
__device__ __forceinline__ void write_partial(const double (&acc)[N], double *__restrict__ ws, int64_t band, int c0, int f) {
    double *rec = ws + band * (N / 4) * (int64_t)f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (c0 + j < f) {
            rec[c0 + j] = acc[j];
            if constexpr (N == 8) rec[f + c0 + j] = acc[4 + j];
        }
}

// Second level, the body of a kernel of final_blocks(R f) blocks: block b owns outputs 32 b .. 32 b + 31 of the R f; group g of
// its threads adds records g, g + 8, ... in that order, then the 8 groups are folded by a fixed tree.  `store(o, v)` runs in the
// one thread that holds output o, v its sum (no record: zero).
template <int R, class Store>
__device__ __forceinline__ void final_sum(const double *__restrict__ ws, int64_t nbands, int f, Store store) {
    __shared__ double sm[kThreads];
    const int tid = threadIdx.x, lane = tid & (kFinalCols - 1), grp = tid / kFinalCols;
    const int o = blockIdx.x * kFinalCols + lane;
    double acc = 0.0;
    if (o < R * f)
        for (int64_t b = grp; b < nbands; b += kFinalGroups) acc += ws[b * R * (int64_t)f + o];
    sm[tid] = acc;
    for (int s = kFinalGroups >> 1; s >= 1; s >>= 1) {
        __syncthreads();
        if (grp < s) sm[tid] += sm[tid + s * kFinalCols];
    }
    if (grp == 0 && o < R * f) store(o, sm[tid]);
}

// ---- host side ----
int log2_threads_per_row(int f) {
    const int quads = (f + 3) / 4;
    int l = 0;
    while ((1 << l) < quads) ++l;
    return l;
}

bool aligned16(const void *p) { return ((uintptr_t)p % 16) == 0; }
bool rows16(int64_t ld) { return ld % 4 == 0; }
int64_t bands(int64_t nrows) { return (nrows + kSumRows - 1) / kSumRows; }
int64_t apply_blocks(int64_t nrows) { return (nrows + kApplyRows - 1) / kApplyRows; }
int64_t final_blocks(int64_t nout) { return (nout + kFinalCols - 1) / kFinalCols; }

// bytes of the work-space of the column sums: one record of `records` x f doubles per band, at least one; -1: not covered
int64_t ws_bytes(int64_t nrows, int32_t f, int records) {
    if (nrows < 0 || f < 1 || f > kMaxF) return -1;
    const int64_t nb = bands(nrows);
    return (nb > 0 ? nb : 1) * records * (int64_t)f * (int64_t)sizeof(double);
}

// One launch of 256-thread blocks; the float4 / scalar pair of a kernel goes in as `vec ? kernel<true> : kernel<false>`.
template <class... P, class... A>
void launch(void (*kernel)(P...), int64_t nblocks, hipStream_t stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblocks), dim3(kThreads), 0, stream, (P)args...);
}

}  // namespace

#endif
