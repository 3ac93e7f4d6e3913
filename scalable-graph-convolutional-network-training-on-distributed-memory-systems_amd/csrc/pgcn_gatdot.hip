// pgcn_gatdot.hip -- the passes of a scaled dot-product attention layer (the layer of the graph transformers: Shi et al., "Masked label
// prediction", IJCAI 2021, without edge features) on the stored entries (gfx950), fp32.  include/pgcn_hip.h has the contract, DESIGN.md
// section 4 the arithmetic and the bytes.
//
//   e_ijk     = s <Zq[i,k,:], Zk[j,k,:]>,  s = 1 / sqrt(d)                                          pgcn_gatdot_scores_f32
//   alpha_i.k = softmax of e_i.k over the stored entries of row i (max subtracted), in place        pgcn_gatv2_softmax_f32 (unchanged)
//   out_i     = sum_j alpha_ij Zv_j                                                                  pgcn_spmm_heads_f32 (unchanged)
//   q_ijk     = <dOut_ik, Zv_jk - out_ik>,  T_ik = sum_j alpha_ijk q_ijk,  de_ijk = alpha_ijk (q_ijk - T_ik)
//   dZq_i     = s sum_j de_ij Zk_j                                                                   pgcn_gatdot_grad_rows_f32
//   dZk_j     = s sum_i de_ij Zq_i,   dZv_j = sum_i alpha_ij dOut_i     (transposed structure)       pgcn_gatdot_grad_cols_f32
//
// The mapping is that of pgcn_gatv2.hip (pgcn_gat_tasks.h): one wave owns a task of the SpMM plan, a lane four features, d / 4 lanes a
// head; the 64 column ids of a stretch are loaded lane-parallel and handed round with a cross-lane read; the other end's rows are
// gathered in unpredicated batches of 8 (an index past the task is clamped to its last entry and its term selected away); per-head dots
// are cross-lane sums (the score's in double, by a transposing reduction: see gatdot_scores_kernel).  Rows cut by the plan leave
// partial rows in slots that pgcn_spmm_fixup_f32 adds in slot order.  Fixed summation order everywhere, no atomics: two runs give the
// same bits.  Plain vector loads and stores.
//
// The row pass is two passes over the forward structure: pass 1 (attn_dalpha_kernel, shared with pgcn_gatv2.hip) writes q into the de
// planes and T, pass 2 forms de = alpha (q - T) from the same q.  pgcn_gat_tasks.h has the kernel and the reason.
//
// The column pass walks the TRANSPOSED structure but reads the FORWARD-order alpha and de planes through the entry permutation
// (perm[p] = the forward position of the transposed structure's entry p): no permuted copies of the planes exist.  The next batch's
// permutation words and plane words are loaded while the current batch's rows are in flight, the next stretch's column ids and
// permutation words while the current stretch is walked.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_gat_tasks.h"      // Plan / Task / Lane, put_row, attn_dalpha_kernel, check_plan / bad_rows: shared with pgcn_gatv2.hip

namespace {

// ---- e = s <Zq_i, Zk_j> ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gatdot_scores_kernel(Plan pl, const float *__restrict__ Zq, int64_t ldq,
                                                                 const float *__restrict__ Zk, int64_t ldk, int32_t d, int32_t F, double s,
                                                                 float *__restrict__ E, int64_t stride) {
    const Task t = pick_task(pl);
    if (!t.act || t.len <= 0) return;          // (wave-uniform; no workgroup barrier below)
    const int lane = threadIdx.x & 63;
    const Lane l = pick_lane(F, d);
    const int hl = d >> 2;
    float zq[4] = {0.f, 0.f, 0.f, 0.f};
    if (l.fact) vload<4>(zq, Zq + t.row * ldq + l.fcol);
    float *ek = E + (int64_t)l.head * stride + t.kbeg;
    const int last = t.len - 1;
    for (int base = 0; base < t.len; base += 64) {
        const int el = base + lane < last ? base + lane : last;
        const int32_t cl = pl.col[t.kbeg + el];
        const int cnt = min(64, t.len - base);
        for (int e0 = 0; e0 < cnt; e0 += kBatch) {
            float x[kBatch][4];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int e = e0 + u < cnt ? e0 + u : cnt - 1;       // ragged tail: the task's last referenced row
                const int32_t c = __shfl(cl, e, 64);
                vload<4>(x[u], Zk + (int64_t)c * ldk + l.fsafe);
            }
            // The dot is formed in DOUBLE (the products of two floats are exact there) and rounded once.  The score is the one quantity
            // whose ABSOLUTE error enters an exponential, and a float32 dot loses eps * sum_c |Zq_c Zk_c|, not eps * |e|: with
            // projections of magnitude 13 and opposing terms (the planted features of the whole-model tests) that error came back
            // through the weight gradients three times larger than the float32 statement's own ("Measured").
            double p[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u)
                p[u] = ((double)zq[0] * (double)x[u][0] + (double)zq[1] * (double)x[u][1]) +
                       ((double)zq[2] * (double)x[u][2] + (double)zq[3] * (double)x[u][3]);
            // 8 entries x hl lanes: a transposing reduction -- each of the first three steps halves the entries a lane carries while it
            // doubles the lanes summed (4 + 2 + 1 exchanges of a double instead of 3 x 8), after which lane L holds entry L & 7 summed
            // over its group of 8 lanes; the head's remaining groups are added with one exchange per step.  (hl >= 8, a power of two.)
            const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
            double r4[4], r2[2];
#pragma unroll
            for (int k = 0; k < 4; ++k) r4[k] = (b0 ? p[2 * k + 1] : p[2 * k]) + __shfl_xor(b0 ? p[2 * k] : p[2 * k + 1], 1, 64);
#pragma unroll
            for (int k = 0; k < 2; ++k) r2[k] = (b1 ? r4[2 * k + 1] : r4[2 * k]) + __shfl_xor(b1 ? r4[2 * k] : r4[2 * k + 1], 2, 64);
            double pm = (b2 ? r2[1] : r2[0]) + __shfl_xor(b2 ? r2[0] : r2[1], 4, 64);
            for (int o = 8; o < hl; o <<= 1) pm += __shfl_xor(pm, o, 64);
            const int e = e0 + l.sub;          // lane `sub` < 8 of a head writes entry `sub` of the batch
            if (l.fact && l.sub < kBatch && e < cnt) ek[base + e] = (float)(s * pm);
        }
    }
}

// ---- pass 2: de = alpha (q - T) in place, dZq_i = s sum_j de_ij Zk_j (row i owns the work) ----------------------------------------------
__global__ __launch_bounds__(kThreads) void gatdot_grad_rows_kernel(Plan pl, const float *__restrict__ Zk, int64_t ldk,
                                                                    const float *__restrict__ alpha, int64_t stride_a,
                                                                    const float *__restrict__ T, int32_t heads, int32_t d, int32_t F, float s,
                                                                    float *__restrict__ de, int64_t stride_de, float *__restrict__ dZq,
                                                                    int64_t ldz, float *__restrict__ partial, uint32_t flags) {
    const Task t = pick_task(pl);
    if (!t.act) return;                        // (wave-uniform; no workgroup barrier below)
    const int lane = threadIdx.x & 63;
    const Lane l = pick_lane(F, d);
    const float ti = l.fact ? T[t.row * heads + l.head] : 0.f;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float *ak = alpha + (int64_t)l.head * stride_a + t.kbeg;
    float *dk = de + (int64_t)l.head * stride_de + t.kbeg;
    const int last = t.len > 0 ? t.len - 1 : 0;
    for (int base = 0; base < t.len; base += 64) {       // wave-uniform: one task per wave
        const int el = base + lane < last ? base + lane : last;
        const int32_t cl = pl.col[t.kbeg + el];
        const int cnt = min(64, t.len - base);
        for (int e0 = 0; e0 < cnt; e0 += kBatch) {
            float x[kBatch][4], al[kBatch], p[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int e = e0 + u < cnt ? e0 + u : cnt - 1;
                const int32_t c = __shfl(cl, e, 64);
                vload<4>(x[u], Zk + (int64_t)c * ldk + l.fsafe);
                al[u] = ak[base + e];
                p[u] = dk[base + e];                                 // q of pass 1 (read by every lane of the head before its writer stores de)
            }
            float gm = 0.f;
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const bool in = e0 + u < cnt;
                const float g = in ? al[u] * (p[u] - ti) : 0.f;      // de of entry u, on every lane of the head
                gm = l.sub == u ? g : gm;
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[v] += in ? g * x[u][v] : 0.f;
            }
            const int e = e0 + l.sub;
            if (l.fact && l.sub < kBatch && e < cnt) dk[base + e] = gm;
        }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[v] *= s;
    put_row(t, l, acc, dZq, ldz, partial, F, flags);
}

// ---- dZk and dZv over the transposed structure (row j owns the work, its columns are the attending i) -------------------------------------
__global__ __launch_bounds__(kThreads) void gatdot_grad_cols_kernel(Plan pl, const int64_t *__restrict__ perm, const float *__restrict__ Zq,
                                                                    int64_t ldq, const float *__restrict__ dOut, int64_t ldo,
                                                                    const float *__restrict__ alpha, int64_t stride_a,
                                                                    const float *__restrict__ de, int64_t stride_de, int32_t d, int32_t F,
                                                                    float s, float *__restrict__ dZk, int64_t ldzk, float *__restrict__ dZv,
                                                                    int64_t ldzv, float *__restrict__ partial_k, float *__restrict__ partial_v,
                                                                    uint32_t flags) {
    const Task t = pick_task(pl);
    if (!t.act) return;                        // (wave-uniform; no workgroup barrier below)
    const int lane = threadIdx.x & 63;
    const Lane l = pick_lane(F, d);
    float acck[4] = {0.f, 0.f, 0.f, 0.f}, accv[4] = {0.f, 0.f, 0.f, 0.f};
    const float *ak = alpha + (int64_t)l.head * stride_a;
    const float *dk = de + (int64_t)l.head * stride_de;
    const int last = t.len > 0 ? t.len - 1 : 0;
    // the first stretch's column ids and permutation words: lane-parallel, index clamped into the task
    int32_t ncl = 0;
    int64_t npm = 0;
    if (t.len > 0) {
        const int el = lane < last ? lane : last;
        ncl = pl.col[t.kbeg + el];
        npm = perm[t.kbeg + el];
    }
    for (int base = 0; base < t.len; base += 64) {
        const int32_t cl = ncl;
        const int64_t pm = npm;
        if (base + 64 < t.len) {               // the next stretch's, while this one is walked
            int el = base + 64 + lane;
            el = el < last ? el : last;
            ncl = pl.col[t.kbeg + el];
            npm = perm[t.kbeg + el];
        }
        const int cnt = min(64, t.len - base);
        float nal[kBatch], ndv[kBatch];        // the plane words of the NEXT batch, through the permutation
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int e = u < cnt ? u : cnt - 1;
            const int64_t p = __shfl(pm, e, 64);
            nal[u] = ak[p];
            ndv[u] = dk[p];
        }
        for (int e0 = 0; e0 < cnt; e0 += kBatch) {
            float y[kBatch][4], g[kBatch][4], al[kBatch], dv[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int e = e0 + u < cnt ? e0 + u : cnt - 1;
                const int32_t c = __shfl(cl, e, 64);
                vload<4>(y[u], Zq + (int64_t)c * ldq + l.fsafe);
                vload<4>(g[u], dOut + (int64_t)c * ldo + l.fsafe);
                al[u] = nal[u];
                dv[u] = ndv[u];
            }
            if (e0 + kBatch < cnt) {           // (wave-uniform) the next batch's words go out behind this batch's rows
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    const int e = e0 + kBatch + u < cnt ? e0 + kBatch + u : cnt - 1;
                    const int64_t p = __shfl(pm, e, 64);
                    nal[u] = ak[p];
                    ndv[u] = dk[p];
                }
            }
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const bool in = e0 + u < cnt;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    acck[v] += in ? dv[u] * y[u][v] : 0.f;
                    accv[v] += in ? al[u] * g[u][v] : 0.f;
                }
            }
        }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) acck[v] *= s;
    put_row(t, l, acck, dZk, ldzk, partial_k, F, flags);
    put_row(t, l, accv, dZv, ldzv, partial_v, F, flags);
}

}  // namespace

// ---- host side (plan_grid, check_plan, bad_rows: pgcn_gat_tasks.h) -------------------------------------------------------------------

extern "C" int pgcn_gatdot_scores_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                                      const int64_t *seg, int32_t nslices, const float *Zq, int64_t ldq, const float *Zk, int64_t ldk,
                                      int32_t heads, int32_t d, float *E, int64_t plane_stride, pgcn_stream_t stream) {
    const char *who = "pgcn_gatdot_scores_f32";
    Plan pl{rowptr, col};
    int64_t grid = 0;
    const int rc = check_plan(who, heads, d, nrows, tasks, ntasks, seg, nslices, &pl, &grid);
    if (rc != PGCN_OK) return rc;
    const int64_t F = (int64_t)heads * d;
    if (ldq < F || ldk < F || plane_stride < 0) return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes");
    if (bad_rows(Zq, ldq) || bad_rows(Zk, ldk))
        return pgcn_set_error2(PGCN_EUNSUPPORTED, who, "needs 16-byte aligned operands and leading dimensions % 4 == 0");
    if (grid == 0) return PGCN_OK;
    if (!rowptr || !col || !Zq || !Zk || !E) return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    hipLaunchKernelGGL(gatdot_scores_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, pl, Zq, ldq, Zk, ldk, d, (int32_t)F,
                       1.0 / sqrt((double)d), E, plane_stride);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_gatdot_grad_rows_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                                         const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const float *Zk, int64_t ldk,
                                         const float *Zv, int64_t ldv, const float *alpha, int64_t alpha_stride, const float *dOut,
                                         int64_t ldo, const float *out, int64_t ldout, float *t_ws, int32_t heads, int32_t d, float *de,
                                         int64_t de_stride, float *dZq, int64_t ldz, float *partial_ws, int64_t partial_ws_elems,
                                         int64_t nslots, uint32_t flags, pgcn_stream_t stream) {
    const char *who = "pgcn_gatdot_grad_rows_f32";
    Plan pl{rowptr, col};
    int64_t grid = 0;
    const int rc = check_plan(who, heads, d, nrows, tasks, ntasks, seg, nslices, &pl, &grid);
    if (rc != PGCN_OK) return rc;
    const int64_t F = (int64_t)heads * d;
    if (ldk < F || ldv < F || ldo < F || ldout < F || ldz < F || nfix < 0 || nslots < 0 || alpha_stride < 0 || de_stride < 0)
        return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes");
    if (bad_rows(Zk, ldk) || bad_rows(Zv, ldv) || bad_rows(dOut, ldo) || bad_rows(out, ldout) || bad_rows(dZq, ldz) ||
        (uintptr_t)partial_ws % 16)
        return pgcn_set_error2(PGCN_EUNSUPPORTED, who, "needs 16-byte aligned operands and leading dimensions % 4 == 0");
    if (grid == 0) return PGCN_OK;
    if (!rowptr || !col || !Zk || !Zv || !alpha || !dOut || !out || !t_ws || !de || !dZq || (nfix > 0 && !fix) || (nslots > 0 && !partial_ws))
        return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    if (partial_ws_elems < nslots * F) return pgcn_set_error2(PGCN_ENOMEM, who, "partial work-space too small");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(attn_dalpha_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, pl, Zv, ldv, alpha, alpha_stride, dOut, ldo, out, ldout,
                       heads, d, (int32_t)F, de, de_stride, t_ws, partial_ws);
    PGCN_HIP_CHECK(hipGetLastError());
    if (nfix > 0) {                            // T of the cut rows, in slot order, before pass 2 takes the slots for dZq
        const int rcf = pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_ws, t_ws, heads, heads, 0, stream);
        if (rcf != PGCN_OK) return rcf;
    }
    hipLaunchKernelGGL(gatdot_grad_rows_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, pl, Zk, ldk, alpha, alpha_stride, t_ws, heads, d,
                       (int32_t)F, 1.0f / sqrtf((float)d), de, de_stride, dZq, ldz, partial_ws, flags);
    PGCN_HIP_CHECK(hipGetLastError());
    if (nfix > 0)
        return pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_ws, dZq, ldz, (int32_t)F, flags & PGCN_SPMM_ACCUMULATE, stream);
    return PGCN_OK;
}

extern "C" int pgcn_gatdot_grad_cols_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                                         const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const int64_t *perm,
                                         const float *Zq, int64_t ldq, const float *dOut, int64_t ldo, const float *alpha,
                                         int64_t alpha_stride, const float *de, int64_t de_stride, int32_t heads, int32_t d, float *dZk,
                                         int64_t ldzk, float *dZv, int64_t ldzv, float *partial_ws, int64_t partial_ws_elems, int64_t nslots,
                                         uint32_t flags, pgcn_stream_t stream) {
    const char *who = "pgcn_gatdot_grad_cols_f32";
    Plan pl{rowptr, col};
    int64_t grid = 0;
    const int rc = check_plan(who, heads, d, nrows, tasks, ntasks, seg, nslices, &pl, &grid);
    if (rc != PGCN_OK) return rc;
    const int64_t F = (int64_t)heads * d;
    if (ldq < F || ldo < F || ldzk < F || ldzv < F || nfix < 0 || nslots < 0 || alpha_stride < 0 || de_stride < 0)
        return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes");
    if (bad_rows(Zq, ldq) || bad_rows(dOut, ldo) || bad_rows(dZk, ldzk) || bad_rows(dZv, ldzv) || (uintptr_t)partial_ws % 16)
        return pgcn_set_error2(PGCN_EUNSUPPORTED, who, "needs 16-byte aligned operands and leading dimensions % 4 == 0");
    if (grid == 0) return PGCN_OK;
    if (!rowptr || !col || !perm || !Zq || !dOut || !alpha || !de || !dZk || !dZv || (nfix > 0 && !fix) || (nslots > 0 && !partial_ws))
        return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    if (partial_ws_elems < 2 * nslots * F) return pgcn_set_error2(PGCN_ENOMEM, who, "partial work-space too small (2 x nslots x heads * d floats)");
    float *partial_v = partial_ws ? partial_ws + nslots * F : nullptr;       // the slot rows of dZv behind those of dZk
    hipLaunchKernelGGL(gatdot_grad_cols_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, pl, perm, Zq, ldq, dOut, ldo,
                       alpha, alpha_stride, de, de_stride, d, (int32_t)F, 1.0f / sqrtf((float)d), dZk, ldzk, dZv, ldzv, partial_ws, partial_v,
                       flags);
    PGCN_HIP_CHECK(hipGetLastError());
    if (nfix > 0) {
        const int rcf = pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_ws, dZk, ldzk, (int32_t)F, flags & PGCN_SPMM_ACCUMULATE, stream);
        if (rcf != PGCN_OK) return rcf;
        return pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_v, dZv, ldzv, (int32_t)F, flags & PGCN_SPMM_ACCUMULATE, stream);
    }
    return PGCN_OK;
}
