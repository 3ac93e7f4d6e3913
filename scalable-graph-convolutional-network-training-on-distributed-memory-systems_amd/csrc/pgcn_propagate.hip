// pgcn_propagate.hip -- the element-wise half of a step of personalised-PageRank propagation (APPNP: predict, then propagate) and of
// its adjoint, for gfx950 (PGCN.py: PPropagate; engine.py: AggregationEngine.propagate / propagate_backward; include/pgcn_hip.h has
// the contract).  The aggregation S = A Z (T = A^T G) is the engine's; these kernels are what follows it, one pass each.
//
//   forward    Y = fl(fl(b S) + fl(a H))                                            pgcn_ppr_step_f32           (one launch)
//   backward   acc = D ? fl(D + fl(a G)) : fl(a G)                                   pgcn_ppr_step_backward_f32  (one launch)
//              last == 0:  Dout = acc,  Gout = fl(b T)
//              last != 0:  Dout = fl(acc + fl(b T))          (the input gradient; Gout is not written)
//
// a = float(alpha) and b = 1.0f - a are formed on the host, once, in fp32.  Every operation is rounded on its own: this file is
// compiled with -ffp-contract=off (csrc/build.sh), the float4 body and the scalar body leave the same bits.  The layout is that of
// pgcn_rowband.h.  Raw pointers + a stream, no allocation, no synchronisation: graph-capturable.  A thread reads its own elements
// before it writes them, so Y may be S, Gout may be T and Dout may be D.  Contiguous operands of a width that is no multiple of 4 run
// as rows of 128 columns (flat_view below): the same bits, float4 traffic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"
#include "pgcn_rowband.h"

namespace {

constexpr int kRowsInFlight = 4;

template <bool VEC>
__global__ __launch_bounds__(kThreads) void step_kernel(const float *S, int64_t lds, const float *H, int64_t ldh, int64_t nrows, int f,
                                                        int log2_tpr, float a, float b, float *Y, int64_t ldy) {
#pragma clang fp contract(off)
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kApplyRows, nrows);
    if (c0 >= f) return;
    for (int64_t r = r0 + rg; r < rend; r += kRowsInFlight * (int64_t)ngroups) {
        Quad s[kRowsInFlight], h[kRowsInFlight];
#pragma unroll
        for (int k = 0; k < kRowsInFlight; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr < rend) {
                s[k] = load_quad<VEC>(S + rr * lds, c0, f);
                h[k] = load_quad<VEC>(H + rr * ldh, c0, f);
            }
        }
#pragma unroll
        for (int k = 0; k < kRowsInFlight; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr >= rend) break;
            Quad y;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float bs = b * s[k].v[j], ah = a * h[k].v[j];
                y.v[j] = bs + ah;
            }
            store_quad<VEC>(Y + rr * ldy, c0, f, y);
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void step_backward_kernel(const float *G, int64_t ldg, const float *T, int64_t ldt, const float *D,
                                                                 int64_t ldd, int64_t nrows, int f, int log2_tpr, float a, float b, int last,
                                                                 float *Gout, int64_t ldgo, float *Dout, int64_t lddo) {
#pragma clang fp contract(off)
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kApplyRows, nrows);
    if (c0 >= f) return;
    const bool has_d = D != nullptr;
    for (int64_t r = r0 + rg; r < rend; r += kRowsInFlight * (int64_t)ngroups) {
        Quad g[kRowsInFlight], t[kRowsInFlight], d[kRowsInFlight];
#pragma unroll
        for (int k = 0; k < kRowsInFlight; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr < rend) {
                g[k] = load_quad<VEC>(G + rr * ldg, c0, f);
                t[k] = load_quad<VEC>(T + rr * ldt, c0, f);
                if (has_d) d[k] = load_quad<VEC>(D + rr * ldd, c0, f);
                else d[k] = Quad{{0.f, 0.f, 0.f, 0.f}};
            }
        }
#pragma unroll
        for (int k = 0; k < kRowsInFlight; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr >= rend) break;
            Quad od, og;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float ag = a * g[k].v[j], bt = b * t[k].v[j];
                const float acc = has_d ? d[k].v[j] + ag : ag;       // (an absent D is not added at all: a -0.0 survives)
                od.v[j] = last ? acc + bt : acc;
                og.v[j] = bt;
            }
            store_quad<VEC>(Dout + rr * lddo, c0, f, od);
            if (!last) store_quad<VEC>(Gout + rr * ldgo, c0, f, og);
        }
    }
}

// alpha in [0, 1) and finite (a NaN fails both comparisons)
bool alpha_ok(float a) { return a >= 0.f && a < 1.f; }

// Contiguous operands (every leading dimension == f) of a width that is no multiple of 4 -- a class count such as 41 -- are the same
// elements as rows of kFlatWidth columns plus one short last row: the work is element-wise, so every element gets the same
// arithmetic and the same bits, and all but that last row moves as float4 instead of guarded scalars (measured at 232 965 x 41:
// DESIGN.md section 4).  The same kernels, launched on that view.
constexpr int kFlatWidth = 128;
bool flat_view(int64_t nrows, int f) { return f % 4 != 0 && nrows > 1; }

void launch_step(const float *S, int64_t lds, const float *H, int64_t ldh, int64_t nrows, int f, float a, float b, float *Y, int64_t ldy,
                 hipStream_t stream) {
    const bool vec = f % 4 == 0 && rows16(lds) && rows16(ldh) && rows16(ldy) && aligned16(S) && aligned16(H) && aligned16(Y);
    launch(vec ? step_kernel<true> : step_kernel<false>, apply_blocks(nrows), stream, S, lds, H, ldh, nrows, f, log2_threads_per_row(f), a,
           b, Y, ldy);
}

void launch_step_backward(const float *G, int64_t ldg, const float *T, int64_t ldt, const float *D, int64_t ldd, int64_t nrows, int f,
                          float a, float b, int last, float *Gout, int64_t ldgo, float *Dout, int64_t lddo, hipStream_t stream) {
    const bool vec = f % 4 == 0 && rows16(ldg) && rows16(ldt) && rows16(lddo) && aligned16(G) && aligned16(T) && aligned16(Dout) &&
                     (!D || (rows16(ldd) && aligned16(D))) && (last || (rows16(ldgo) && aligned16(Gout)));
    launch(vec ? step_backward_kernel<true> : step_backward_kernel<false>, apply_blocks(nrows), stream, G, ldg, T, ldt, D, ldd, nrows, f,
           log2_threads_per_row(f), a, b, last, Gout, ldgo, Dout, lddo);
}

}  // namespace

extern "C" int pgcn_ppr_step_f32(const float *S, int64_t lds, const float *H, int64_t ldh, int64_t nrows, int32_t f, float alpha, float *Y,
                                 int64_t ldy, pgcn_stream_t stream) {
    if (nrows < 0 || f < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_ppr_step_f32: nrows < 0 or f < 1");
    if (nrows > 0 && (!S || !H || !Y)) return pgcn_set_error(PGCN_EINVAL, "pgcn_ppr_step_f32: null pointer");
    if (lds < f || ldh < f || ldy < f) return pgcn_set_error(PGCN_EINVAL, "pgcn_ppr_step_f32: a leading dimension is below f");
    if (Y && ((Y == S && ldy != lds) || (Y == H && ldy != ldh)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_ppr_step_f32: in place (Y == S or Y == H) needs equal leading dimensions");
    if (!alpha_ok(alpha)) return pgcn_set_error(PGCN_EINVAL, "pgcn_ppr_step_f32: alpha must be finite and in [0, 1)");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_ppr_step_f32: more than 1024 columns");
    if (nrows == 0) return PGCN_OK;
    const float a = alpha, b = 1.0f - a;
    hipStream_t s = (hipStream_t)stream;
    if (flat_view(nrows, f) && lds == f && ldh == f && ldy == f) {
        const int64_t total = nrows * (int64_t)f, rows = total / kFlatWidth, done = rows * kFlatWidth;
        const int rest = (int)(total - done);
        if (rows > 0) launch_step(S, kFlatWidth, H, kFlatWidth, rows, kFlatWidth, a, b, Y, kFlatWidth, s);
        if (rest > 0) launch_step(S + done, rest, H + done, rest, 1, rest, a, b, Y + done, rest, s);
    } else {
        launch_step(S, lds, H, ldh, nrows, f, a, b, Y, ldy, s);
    }
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_ppr_step_backward_f32(const float *G, int64_t ldg, const float *T, int64_t ldt, const float *D, int64_t ldd,
                                          int64_t nrows, int32_t f, float alpha, int32_t last, float *Gout, int64_t ldgo, float *Dout,
                                          int64_t lddo, pgcn_stream_t stream) {
    if (nrows < 0 || f < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_ppr_step_backward_f32: nrows < 0 or f < 1");
    if (nrows > 0 && (!G || !T || !Dout || (!last && !Gout))) return pgcn_set_error(PGCN_EINVAL, "pgcn_ppr_step_backward_f32: null pointer");
    if (ldg < f || ldt < f || lddo < f || (D && ldd < f) || (!last && ldgo < f))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_ppr_step_backward_f32: a leading dimension is below f");
    if (!last && Gout && ((Gout == T && ldgo != ldt) || (Gout == G && ldgo != ldg)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_ppr_step_backward_f32: in place (Gout == T or Gout == G) needs equal leading dimensions");
    if (Dout && ((Dout == D && lddo != ldd) || (Dout == G && lddo != ldg) || (Dout == T && lddo != ldt)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_ppr_step_backward_f32: in place (Dout == D, G or T) needs equal leading dimensions");
    if (!last && Gout && Gout == Dout) return pgcn_set_error(PGCN_EINVAL, "pgcn_ppr_step_backward_f32: Gout and Dout are the same matrix");
    if (!alpha_ok(alpha)) return pgcn_set_error(PGCN_EINVAL, "pgcn_ppr_step_backward_f32: alpha must be finite and in [0, 1)");
    if (f > kMaxF) return pgcn_set_error(PGCN_EUNSUPPORTED, "pgcn_ppr_step_backward_f32: more than 1024 columns");
    if (nrows == 0) return PGCN_OK;
    const float a = alpha, b = 1.0f - a;
    hipStream_t s = (hipStream_t)stream;
    const int is_last = last != 0;
    if (flat_view(nrows, f) && ldg == f && ldt == f && lddo == f && (!D || ldd == f) && (is_last || ldgo == f)) {
        const int64_t total = nrows * (int64_t)f, rows = total / kFlatWidth, done = rows * kFlatWidth;
        const int rest = (int)(total - done);
        float *go = is_last ? nullptr : Gout;          // (not written at the last step: may be NULL, is never offset)
        if (rows > 0)
            launch_step_backward(G, kFlatWidth, T, kFlatWidth, D, kFlatWidth, rows, kFlatWidth, a, b, is_last, go, kFlatWidth, Dout, kFlatWidth, s);
        if (rest > 0)
            launch_step_backward(G + done, rest, T + done, rest, D ? D + done : nullptr, rest, 1, rest, a, b, is_last, go ? go + done : nullptr,
                                 rest, Dout + done, rest, s);
    } else {
        launch_step_backward(G, ldg, T, ldt, D, ldd, nrows, f, a, b, is_last, Gout, ldgo, Dout, lddo, s);
    }
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}
