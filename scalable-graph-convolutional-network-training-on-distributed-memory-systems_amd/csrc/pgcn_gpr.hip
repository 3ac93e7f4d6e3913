// pgcn_gpr.hip -- the element-wise half of a step of the generalised-PageRank propagation with learned hop weights (GPR-GNN, Chien
// et al., ICLR 2021) and of its adjoint, for gfx950 (PGCN.py: PGpr; engine.py: AggregationEngine.gpr / gpr_backward;
// include/pgcn_hip.h has the contract).  OUT = sum_{k=0..K} g_k A^k H: the aggregations S^k = A S^{k-1} (T^k = A^T T^{k-1}) are the
// engine's; these kernels are what follows each of them, one pass each.
//
//   forward    Y = Yin ? fl(Yin + fl(g_k X)) : fl(g_k X)                             pgcn_gpr_step_f32           (one launch)
//   backward   Dout = Din ? fl(Din + fl(g_k T)) : fl(g_k T)   (Dout NULL: skipped)   pgcn_gpr_step_backward_f32  (one launch)
//              and, in the same pass, the band's partial of sum_{i,c} (double)T[i,c] (double)H[i,c] to the work-space
//   finish     dgamma[k] = float(sum of the k-th region's band records), k = 0 .. K  pgcn_gpr_dot_finish_f32     (one launch)
//
// g = gamma is K + 1 floats in DEVICE memory, read by the kernels: an optimiser step needs no rebinding and the host never reads
// it.  Every operation is rounded on its own: this file is compiled with -ffp-contract=off (csrc/build.sh), the float4 body and the
// scalar body leave the same bits.  The layout, fold_row_groups, write_partial and final_sum are those of pgcn_rowband.h.  The
// product of two floats is exact in double; a thread adds its products in double in row order, the row groups of a band of kSumRows
// rows are folded by the fixed tree of fold_row_groups, the columns by a second fixed tree, and the band leaves ONE double.  The
// work-space holds K + 1 regions of 1 + slots doubles: word 0 of region k is the number of records the step k wrote (an int64, by the
// kernel), the records follow in band order.  The finish adds a region's records in ascending order with final_sum's tree and
// rounds once.  No floating-point atomics: the same input gives the same bits.  A NaN or inf stays in its own element and its own
// dgamma[k].  Raw pointers + a stream, no allocation, no synchronisation: graph-capturable.  A thread reads its own elements before
// it writes them, so Y may be Yin (or X) and Dout may be Din (or T).  Contiguous operands of a width that is no multiple of 4 run as
// rows of 128 columns (flat_view below): element-wise work and a sum over ALL elements, the same bits of Y and D, float4 traffic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"
#include "pgcn_rowband.h"

namespace {

constexpr int kRowsInFlight = 4;
constexpr int kMaxK = 65534;           // (the finish runs one block per k in the grid's y)

template <bool VEC>
__global__ __launch_bounds__(kThreads) void step_kernel(const float *X, int64_t ldx, const float *Yin, int64_t ldyin,
                                                        const float *__restrict__ gamma, int k, int64_t nrows, int f, int log2_tpr,
                                                        float *Y, int64_t ldy) {
#pragma clang fp contract(off)
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kApplyRows, nrows);
    if (c0 >= f) return;
    const float g = gamma[k];
    const bool has_in = Yin != nullptr;
    for (int64_t r = r0 + rg; r < rend; r += kRowsInFlight * (int64_t)ngroups) {
        Quad x[kRowsInFlight], y[kRowsInFlight];
#pragma unroll
        for (int q = 0; q < kRowsInFlight; ++q) {
            const int64_t rr = r + (int64_t)q * ngroups;
            if (rr < rend) {
                x[q] = load_quad<VEC>(X + rr * ldx, c0, f);
                if (has_in) y[q] = load_quad<VEC>(Yin + rr * ldyin, c0, f);
                else y[q] = Quad{{0.f, 0.f, 0.f, 0.f}};
            }
        }
#pragma unroll
        for (int q = 0; q < kRowsInFlight; ++q) {
            const int64_t rr = r + (int64_t)q * ngroups;
            if (rr >= rend) break;
            Quad o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float gx = g * x[q].v[j];
                o.v[j] = has_in ? y[q].v[j] + gx : gx;              // (an absent Yin is not added at all: a -0.0 survives)
            }
            store_quad<VEC>(Y + rr * ldy, c0, f, o);
        }
    }
}

// One pass over T and H (and Din): writes Dout (Dout != NULL) and record `rec0 + blockIdx.x` of the region `ws`; the block that
// holds the last band of the call also writes the region's record count when `count` >= 0.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void step_backward_kernel(const float *T, int64_t ldt, const float *__restrict__ H, int64_t ldh,
                                                                 const float *Din, int64_t lddin, const float *__restrict__ gamma, int k,
                                                                 int64_t nrows, int f, int log2_tpr, float *Dout, int64_t lddo,
                                                                 double *__restrict__ ws, int64_t rec0, int64_t count) {
#pragma clang fp contract(off)
    __shared__ double sm[4 * kThreads];
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kSumRows, nrows);
    const bool active = c0 < f, has_in = Din != nullptr, has_out = Dout != nullptr;
    double acc[4] = {0, 0, 0, 0};
    if (active) {
        const float g = gamma[k];
        for (int64_t r = r0 + rg; r < rend; r += kRowsInFlight * (int64_t)ngroups) {
            Quad t[kRowsInFlight], h[kRowsInFlight], d[kRowsInFlight];
#pragma unroll
            for (int q = 0; q < kRowsInFlight; ++q) {
                const int64_t rr = r + (int64_t)q * ngroups;
                if (rr < rend) {
                    t[q] = load_quad<VEC>(T + rr * ldt, c0, f);
                    h[q] = load_quad<VEC>(H + rr * ldh, c0, f);
                    if (has_in && has_out) d[q] = load_quad<VEC>(Din + rr * lddin, c0, f);
                    else d[q] = Quad{{0.f, 0.f, 0.f, 0.f}};
                }
            }
#pragma unroll
            for (int q = 0; q < kRowsInFlight; ++q) {
                const int64_t rr = r + (int64_t)q * ngroups;
                if (rr >= rend) break;
                Quad o;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float gt = g * t[q].v[j];
                    o.v[j] = has_in ? d[q].v[j] + gt : gt;
                    // (exact in double; a lane beyond the last column loaded zeros: it adds zeros and stores nothing)
                    acc[j] += (double)t[q].v[j] * (double)h[q].v[j];
                }
                if (has_out) store_quad<VEC>(Dout + rr * lddo, c0, f, o);
            }
        }
    }
    fold_row_groups(acc, sm, log2_tpr);                  // row group 0 holds the band's column sums
    // the columns: a thread's four in index order, then the row's threads by a fixed tree
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < tpr) sm[tid] = ((acc[0] + acc[1]) + acc[2]) + acc[3];
    for (int s = tpr >> 1; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) sm[tid] += sm[tid + s];
    }
    __syncthreads();
    double one[4] = {sm[0], 0, 0, 0};
    if (tid == 0) {
        write_partial(one, ws + 1, rec0 + blockIdx.x, 0, 1);
        if (count >= 0 && blockIdx.x == gridDim.x - 1) *reinterpret_cast<int64_t *>(ws) = count;
    }
}

// Block (0, k) adds the records of region k.  `empty`: no step ran (no rows), every sum is zero.
__global__ __launch_bounds__(kThreads) void finish_kernel(const double *__restrict__ ws, int64_t stride, int64_t slots, int empty,
                                                          float *__restrict__ dgamma) {
    const int k = blockIdx.y;
    const double *region = ws + (int64_t)k * stride;
    int64_t nb = empty ? 0 : *reinterpret_cast<const int64_t *>(region);
    nb = nb < 0 ? 0 : (nb > slots ? slots : nb);         // (a region no step wrote holds anything: never read past it)
    final_sum<1>(region + 1, nb, 1, [=](int o, double v) { dgamma[k + o] = (float)v; });
}

// Contiguous operands (every leading dimension == f) of a width that is no multiple of 4, as in pgcn_propagate.hip: rows of
// kFlatWidth columns plus one short last row.
constexpr int kFlatWidth = 128;
bool flat_view(int64_t nrows, int f) { return f % 4 != 0 && nrows > 1; }

// records a backward step may write: the bands of the plain view, or of the flat view and its short row
int64_t slots_of(int64_t nrows, int f) {
    const int64_t plain = bands(nrows), flat = f % 4 != 0 ? bands(nrows * (int64_t)f / kFlatWidth) + 1 : 0;
    const int64_t s = plain > flat ? plain : flat;
    return s > 0 ? s : 1;
}

void launch_step(const float *X, int64_t ldx, const float *Yin, int64_t ldyin, const float *gamma, int k, int64_t nrows, int f, float *Y,
                 int64_t ldy, hipStream_t stream) {
    const bool vec = f % 4 == 0 && rows16(ldx) && rows16(ldy) && aligned16(X) && aligned16(Y) && (!Yin || (rows16(ldyin) && aligned16(Yin)));
    launch(vec ? step_kernel<true> : step_kernel<false>, apply_blocks(nrows), stream, X, ldx, Yin, ldyin, gamma, k, nrows, f,
           log2_threads_per_row(f), Y, ldy);
}

void launch_step_backward(const float *T, int64_t ldt, const float *H, int64_t ldh, const float *Din, int64_t lddin, const float *gamma,
                          int k, int64_t nrows, int f, float *Dout, int64_t lddo, double *region, int64_t rec0, int64_t count,
                          hipStream_t stream) {
    const bool vec = f % 4 == 0 && rows16(ldt) && rows16(ldh) && aligned16(T) && aligned16(H) &&
                     (!Dout || (rows16(lddo) && aligned16(Dout) && (!Din || (rows16(lddin) && aligned16(Din)))));
    launch(vec ? step_backward_kernel<true> : step_backward_kernel<false>, bands(nrows), stream, T, ldt, H, ldh, Din, lddin, gamma, k, nrows,
           f, log2_threads_per_row(f), Dout, lddo, region, rec0, count);
}

}  // namespace

extern "C" int64_t pgcn_gpr_ws_bytes(int64_t nrows, int32_t f, int32_t K) {
    if (nrows < 0 || f < 1 || f > kMaxF || K < 0 || K > kMaxK) return -1;
    return ((int64_t)K + 1) * (1 + slots_of(nrows, f)) * (int64_t)sizeof(double);
}

extern "C" int pgcn_gpr_step_f32(const float *X, int64_t ldx, const float *Yin, int64_t ldyin, const float *gamma, int32_t k, int32_t K,
                                 int64_t nrows, int32_t f, float *Y, int64_t ldy, pgcn_stream_t stream) {
    if (nrows < 0 || f < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_step_f32: nrows < 0 or f < 1");
    if (K < 0 || K > kMaxK || k < 0 || k > K) return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_step_f32: k outside 0 .. K");
    if (!gamma || (nrows > 0 && (!X || !Y))) return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_step_f32: null pointer");
    if (ldx < f || ldy < f || (Yin && ldyin < f)) return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_step_f32: a leading dimension is below f");
    if (Y && ((Y == Yin && ldy != ldyin) || (Y == X && ldy != ldx)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_step_f32: in place (Y == Yin or Y == X) needs equal leading dimensions");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_gpr_step_f32: more than 1024 columns");
    if (nrows == 0) return PGCN_OK;
    hipStream_t s = (hipStream_t)stream;
    if (flat_view(nrows, f) && ldx == f && ldy == f && (!Yin || ldyin == f)) {
        const int64_t total = nrows * (int64_t)f, rows = total / kFlatWidth, done = rows * kFlatWidth;
        const int rest = (int)(total - done);
        if (rows > 0) launch_step(X, kFlatWidth, Yin, kFlatWidth, gamma, k, rows, kFlatWidth, Y, kFlatWidth, s);
        if (rest > 0) launch_step(X + done, rest, Yin ? Yin + done : nullptr, rest, gamma, k, 1, rest, Y + done, rest, s);
    } else {
        launch_step(X, ldx, Yin, ldyin, gamma, k, nrows, f, Y, ldy, s);
    }
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_gpr_step_backward_f32(const float *T, int64_t ldt, const float *H, int64_t ldh, const float *Din, int64_t lddin,
                                          const float *gamma, int32_t k, int32_t K, int64_t nrows, int32_t f, float *Dout, int64_t lddo,
                                          void *ws, int64_t ws_bytes, pgcn_stream_t stream) {
    if (nrows < 0 || f < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_step_backward_f32: nrows < 0 or f < 1");
    if (K < 0 || K > kMaxK || k < 0 || k > K) return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_step_backward_f32: k outside 0 .. K");
    if (!gamma || !ws || (nrows > 0 && (!T || !H))) return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_step_backward_f32: null pointer");
    if ((uintptr_t)ws % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_step_backward_f32: ws must be 8-byte aligned");
    if (ldt < f || ldh < f || (Dout && lddo < f) || (Dout && Din && lddin < f))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_step_backward_f32: a leading dimension is below f");
    if (Dout && ((Dout == Din && lddo != lddin) || (Dout == T && lddo != ldt) || (Dout == H && lddo != ldh)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_step_backward_f32: in place (Dout == Din, T or H) needs equal leading dimensions");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_gpr_step_backward_f32: more than 1024 columns");
    if (ws_bytes < pgcn_gpr_ws_bytes(nrows, f, K)) return pgcn_set_error(PGCN_ENOMEM, "pgcn_gpr_step_backward_f32: work-space too small");
    if (nrows == 0) return PGCN_OK;
    hipStream_t s = (hipStream_t)stream;
    double *region = (double *)ws + (int64_t)k * (1 + slots_of(nrows, f));
    if (!Dout) Din = nullptr;
    if (flat_view(nrows, f) && ldt == f && ldh == f && (!Dout || (lddo == f && (!Din || lddin == f)))) {
        const int64_t total = nrows * (int64_t)f, rows = total / kFlatWidth, done = rows * kFlatWidth;
        const int rest = (int)(total - done);
        const int64_t nb = bands(rows), count = nb + (rest > 0 ? 1 : 0);
        if (rows > 0)
            launch_step_backward(T, kFlatWidth, H, kFlatWidth, Din, kFlatWidth, gamma, k, rows, kFlatWidth, Dout, kFlatWidth, region, 0,
                                 rest > 0 ? -1 : count, s);
        if (rest > 0)
            launch_step_backward(T + done, rest, H + done, rest, Din ? Din + done : nullptr, rest, gamma, k, 1, rest,
                                 Dout ? Dout + done : nullptr, rest, region, nb, count, s);
    } else {
        launch_step_backward(T, ldt, H, ldh, Din, lddin, gamma, k, nrows, f, Dout, lddo, region, 0, bands(nrows), s);
    }
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_gpr_dot_finish_f32(const void *ws, int64_t ws_bytes, int64_t nrows, int32_t f, int32_t K, float *dgamma,
                                       pgcn_stream_t stream) {
    if (nrows < 0 || f < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_dot_finish_f32: nrows < 0 or f < 1");
    if (K < 0 || K > kMaxK) return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_dot_finish_f32: K outside 0 .. 65534");
    if (!ws || !dgamma) return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_dot_finish_f32: null pointer");
    if ((uintptr_t)ws % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_gpr_dot_finish_f32: ws must be 8-byte aligned");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_gpr_dot_finish_f32: more than 1024 columns");
    if (ws_bytes < pgcn_gpr_ws_bytes(nrows, f, K)) return pgcn_set_error(PGCN_ENOMEM, "pgcn_gpr_dot_finish_f32: work-space too small");
    const int64_t slots = slots_of(nrows, f);
    hipLaunchKernelGGL(finish_kernel, dim3(1, (unsigned)(K + 1)), dim3(kThreads), 0, (hipStream_t)stream, (const double *)ws, 1 + slots,
                       slots, nrows == 0 ? 1 : 0, dgamma);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}
