// pgcn_gatv2.hip -- the passes of a GATv2 layer (dynamic attention; Brody, Alon, Yahav, ICLR 2022) on the stored entries (gfx950), fp32.
// include/pgcn_hip.h has the contract, DESIGN.md section 4 the arithmetic and the bytes.
//
//   e_ijk     = sum_c a[c,k] LeakyReLU(Zt[i,k,c] + Zs[j,k,c])                                       pgcn_gatv2_scores_f32
//   alpha_i.k = softmax of e_i.k over the stored entries of row i (max subtracted), in place        pgcn_gatv2_softmax_f32
//   out_i     = sum_j alpha_ij Zs_j                                                                  pgcn_spmm_heads_f32 (unchanged)
//   de_ijk    = alpha_ijk (<dOut_ik, Zs_jk> - t_ik) = alpha_ijk <dOut_ik, Zs_jk - out_ik>      (t_ik = <dOut_ik, out_ik>)
//   dZt_i     = sum_j de_ij a LReLU'(x_ij),   da = sum_ij de_ij LReLU(x_ij)
//                                                                                                    pgcn_gatv2_grad_rows_f32
//   dZs_j     = sum_i (de_ij a LReLU'(x_ij) + alpha_ij dOut_i)     (transposed structure)            pgcn_gatv2_grad_cols_f32
//
// The static score of GAT splits into s1_i + s2_j, two scalars per vertex and head; this one does not: every entry needs both d-wide
// rows.  Scores, alpha and de therefore live in head-major planes [heads][nnz] in the storage order of `col` -- the layout
// pgcn_spmm_heads_f32 consumes -- and every pass walks the tasks of the SpMM plan of its structure.
//
// Mapping to the machine: that of spmm_heads_kernel.  One wave owns a task (a row, an XCD slice of it or a chunk of a long row), a lane
// owns four features of the heads * d <= 256 wide row, d / 4 lanes form a head.  The task's own row and the lane's four elements of `a`
// stay in registers; the 64 column ids of a stretch are loaded lane-parallel and handed round with a cross-lane read; the other end's
// rows are gathered in unpredicated batches of 8 (an index past the task is clamped to its last entry and its term selected away).
// Per-head dots are butterfly sums over the head's lanes.  Rows cut by the plan leave partial rows in slots that pgcn_spmm_fixup_f32
// adds in slot order; da is summed wave -> workgroup (LDS, wave order) -> work-space row per workgroup -> two passes in index order.
// Fixed summation order everywhere, no atomics: two runs give the same bits.  Plain vector loads and stores.
//
// The row pass is TWO passes over the forward structure: pass 1 (attn_dalpha_kernel, shared with pgcn_gatdot.hip) writes q_ij into the
// de planes and T_i, pass 2 forms de_ij = alpha_ij (q_ij - T_i) from the same q.  pgcn_gat_tasks.h has the kernel and the reason.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_gat_tasks.h"      // Plan / Task / Lane, put_row, attn_dalpha_kernel, check_plan / bad_rows: shared with pgcn_gatdot.hip

namespace {

constexpr int kDaGroup = 256;          // work-space rows added per thread in the first pass of the da sum

// the lane's four elements of a [d][heads]
__device__ __forceinline__ void load_a(float (&av)[4], const float *__restrict__ a, const Lane &l, int32_t heads, int32_t d) {
    const int c0 = l.fcol - l.head * d;
#pragma unroll
    for (int v = 0; v < 4; ++v) av[v] = l.fact ? a[(int64_t)(c0 + v) * heads + l.head] : 0.f;
}

__device__ __forceinline__ float head_sum(float v, int hl) {
    for (int o = hl >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- e = a . LeakyReLU(Zt_i + Zs_j) --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gatv2_scores_kernel(Plan pl, const float *__restrict__ Zt, int64_t ldt,
                                                                const float *__restrict__ Zs, int64_t lds, const float *__restrict__ a,
                                                                int32_t heads, int32_t d, int32_t F, float slope, float *__restrict__ E,
                                                                int64_t stride) {
    const Task t = pick_task(pl);
    if (!t.act || t.len <= 0) return;          // (wave-uniform; no workgroup barrier below)
    const int lane = threadIdx.x & 63;
    const Lane l = pick_lane(F, d);
    const int hl = d >> 2;
    float zt[4] = {0.f, 0.f, 0.f, 0.f}, av[4];
    if (l.fact) vload<4>(zt, Zt + t.row * ldt + l.fcol);
    load_a(av, a, l, heads, d);
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
                vload<4>(x[u], Zs + (int64_t)c * lds + l.fsafe);
            }
            float p[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                float s = 0.f;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float xv = zt[v] + x[u][v];
                    s += av[v] * (xv > 0.f ? xv : xv * slope);
                }
                p[u] = s;
            }
            for (int o = hl >> 1; o > 0; o >>= 1) {
#pragma unroll
                for (int u = 0; u < kBatch; ++u) p[u] += __shfl_xor(p[u], o, 64);
            }
            float pm = p[0];
#pragma unroll
            for (int u = 1; u < kBatch; ++u) pm = l.sub == u ? p[u] : pm;
            const int e = e0 + l.sub;          // lane `sub` of a head writes entry `sub` of the batch
            if (l.fact && l.sub < kBatch && e < cnt) ek[base + e] = pm;
        }
    }
}

// ---- alpha = softmax of e over the row, in place ----------------------------------------------------------------------------------
__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// TPR = 64: the caller's wave; TPR = 256: the whole workgroup (4 waves through LDS)
template <int TPR, bool MAX>
__device__ __forceinline__ float group_reduce(float v, float *red) {
    v = MAX ? wave_max(v) : head_sum(v, 64);
    if constexpr (TPR == 64) return v;
    __syncthreads();                       // red[] may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float a = red[0], b = red[1], c = red[2], d = red[3];
    return MAX ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : ((a + b) + (c + d));
}

template <int TPR>
__global__ __launch_bounds__(kThreads) void gatv2_softmax_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ rows,
                                                                 int64_t nlist, float *__restrict__ E, int64_t stride) {
    __shared__ float red[4];
    int64_t li;
    int lane;
    if constexpr (TPR == 64) {
        li = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
        lane = threadIdx.x & 63;
    } else {
        li = blockIdx.x;
        lane = threadIdx.x;
    }
    if (li >= nlist) return;               // (TPR = 256: the same for the whole workgroup)
    const int64_t i = rows ? (int64_t)rows[li] : li;
    const int64_t b = rowptr[i], e = rowptr[i + 1];
    if (e <= b) return;                    // an empty row has no entries to write
    float *p = E + (int64_t)blockIdx.y * stride;
    float m = -INFINITY;
    for (int64_t q = b + lane; q < e; q += TPR) m = fmaxf(m, p[q]);
    m = group_reduce<TPR, true>(m, red);
    float s = 0.f;
    for (int64_t q = b + lane; q < e; q += TPR) {
        const float ex = expf(p[q] - m);
        p[q] = ex;                         // (read back by the thread that wrote it)
        s += ex;
    }
    s = group_reduce<TPR, false>(s, red);  // >= 1: the entry of the maximum contributes exp(0)
    for (int64_t q = b + lane; q < e; q += TPR) p[q] = p[q] / s;
}

// ---- pass 2: de = alpha (q - T) in place, dZt and da (row i owns the work) ------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gatv2_grad_rows_kernel(Plan pl, const float *__restrict__ Zt, int64_t ldt,
                                                                   const float *__restrict__ Zs, int64_t lds, const float *__restrict__ a,
                                                                   const float *__restrict__ alpha, int64_t stride_a,
                                                                   const float *__restrict__ T,
                                                                   int32_t heads, int32_t d, int32_t F, float slope, float *__restrict__ de,
                                                                   int64_t stride_de, float *__restrict__ dZt, int64_t ldz,
                                                                   float *__restrict__ partial, uint32_t flags, float *__restrict__ da_part) {
    __shared__ float red[kWaves][256];
    const Task t = pick_task(pl);
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const Lane l = pick_lane(F, d);
    float zt[4] = {0.f, 0.f, 0.f, 0.f}, av[4];
    float ti = 0.f;
    if (t.act && l.fact) {
        vload<4>(zt, Zt + t.row * ldt + l.fcol);
        ti = T[t.row * heads + l.head];
    }
    load_a(av, a, l, heads, d);
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, dacc[4] = {0.f, 0.f, 0.f, 0.f};
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
                vload<4>(x[u], Zs + (int64_t)c * lds + l.fsafe);
                al[u] = ak[base + e];
                p[u] = dk[base + e];                                 // q of pass 1 (read by every lane of the head before its writer stores de)
            }
            float gm = 0.f;
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const bool in = e0 + u < cnt;
                const float g = al[u] * (p[u] - ti);                 // de of entry u, on every lane of the head
                gm = l.sub == u ? g : gm;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float xv = zt[v] + x[u][v];
                    const bool pos = xv > 0.f;
                    const float ga = g * av[v];
                    acc[v] += in ? (pos ? ga : ga * slope) : 0.f;
                    dacc[v] += in ? g * (pos ? xv : xv * slope) : 0.f;
                }
            }
            const int e = e0 + l.sub;
            if (l.fact && l.sub < kBatch && e < cnt) dk[base + e] = gm;
        }
    }
    put_row(t, l, acc, dZt, ldz, partial, F, flags);
    // da: the workgroup's four waves in wave order, one work-space row per workgroup (a workgroup without tasks writes zeros)
#pragma unroll
    for (int v = 0; v < 4; ++v) red[wave][lane * 4 + v] = (t.act && l.fact) ? dacc[v] : 0.f;
    __syncthreads();
    if ((int)threadIdx.x < F)
        da_part[(int64_t)blockIdx.x * F + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// dst[g][f] = sum over the rows r in [g * per, min(n, (g + 1) * per)) of src[r][f], in index order; `last`: the one row left is
// written as da[c][k] (f = k * d + c)
__global__ __launch_bounds__(kThreads) void gatv2_da_sum_kernel(const float *__restrict__ src, int64_t n, int64_t per, int32_t F,
                                                                int32_t heads, int32_t d, float *__restrict__ dst, int last) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t g = idx / F;
    const int f = (int)(idx - g * F);
    if (g * per >= n) return;
    const int64_t r1 = (g + 1) * per < n ? (g + 1) * per : n;
    float s = 0.f;
    for (int64_t r = g * per; r < r1; ++r) s += src[r * F + f];
    if (last) dst[(int64_t)(f % d) * heads + f / d] = s;
    else dst[g * F + f] = s;
}

// ---- dZs over the transposed structure (row j owns the work, its columns are the attending i) ---------------------------------------
__global__ __launch_bounds__(kThreads) void gatv2_grad_cols_kernel(Plan pl, const float *__restrict__ Zs, int64_t lds,
                                                                   const float *__restrict__ Zt, int64_t ldt, const float *__restrict__ dOut,
                                                                   int64_t ldo, const float *__restrict__ a, const float *__restrict__ alpha_t,
                                                                   int64_t stride_a, const float *__restrict__ de_t, int64_t stride_de,
                                                                   int32_t heads, int32_t d, int32_t F, float slope, float *__restrict__ dZs,
                                                                   int64_t ldz, float *__restrict__ partial, uint32_t flags) {
    const Task t = pick_task(pl);
    if (!t.act) return;                        // (wave-uniform; no workgroup barrier below)
    const int lane = threadIdx.x & 63;
    const Lane l = pick_lane(F, d);
    float zs[4] = {0.f, 0.f, 0.f, 0.f}, av[4];
    if (l.fact) vload<4>(zs, Zs + t.row * lds + l.fcol);
    load_a(av, a, l, heads, d);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float *ak = alpha_t + (int64_t)l.head * stride_a + t.kbeg;
    const float *dk = de_t + (int64_t)l.head * stride_de + t.kbeg;
    const int last = t.len > 0 ? t.len - 1 : 0;
    for (int base = 0; base < t.len; base += 64) {
        const int el = base + lane < last ? base + lane : last;
        const int32_t cl = pl.col[t.kbeg + el];
        const int cnt = min(64, t.len - base);
        for (int e0 = 0; e0 < cnt; e0 += kBatch) {
            float y[kBatch][4], g[kBatch][4], al[kBatch], dv[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int e = e0 + u < cnt ? e0 + u : cnt - 1;
                const int32_t c = __shfl(cl, e, 64);
                vload<4>(y[u], Zt + (int64_t)c * ldt + l.fsafe);
                vload<4>(g[u], dOut + (int64_t)c * ldo + l.fsafe);
                al[u] = ak[base + e];
                dv[u] = dk[base + e];
            }
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const bool in = e0 + u < cnt;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float ga = dv[u] * av[v];
                    const float term = (y[u][v] + zs[v] > 0.f ? ga : ga * slope) + al[u] * g[u][v];
                    acc[v] += in ? term : 0.f;
                }
            }
        }
    }
    put_row(t, l, acc, dZs, ldz, partial, F, flags);
}

}  // namespace

// ---- host side (plan_grid, check_plan, bad_rows: pgcn_gat_tasks.h) -------------------------------------------------------------------

extern "C" int pgcn_gatv2_scores_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                                     const int64_t *seg, int32_t nslices, const float *Zt, int64_t ldt, const float *Zs, int64_t lds,
                                     const float *a, int32_t heads, int32_t d, float slope, float *E, int64_t plane_stride,
                                     pgcn_stream_t stream) {
    const char *who = "pgcn_gatv2_scores_f32";
    Plan pl{rowptr, col};
    int64_t grid = 0;
    const int rc = check_plan(who, heads, d, nrows, tasks, ntasks, seg, nslices, &pl, &grid);
    if (rc != PGCN_OK) return rc;
    const int64_t F = (int64_t)heads * d;
    if (ldt < F || lds < F || plane_stride < 0) return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes");
    if (bad_rows(Zt, ldt) || bad_rows(Zs, lds))
        return pgcn_set_error2(PGCN_EUNSUPPORTED, who, "needs 16-byte aligned operands and leading dimensions % 4 == 0");
    if (grid == 0) return PGCN_OK;
    if (!rowptr || !col || !Zt || !Zs || !a || !E) return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    hipLaunchKernelGGL(gatv2_scores_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, pl, Zt, ldt, Zs, lds, a, heads, d,
                       (int32_t)F, slope, E, plane_stride);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_gatv2_softmax_f32(const int64_t *rowptr, int64_t nrows, const int32_t *rows_wave, int64_t nrows_wave,
                                      const int32_t *rows_block, int64_t nrows_block, int32_t heads, float *E, int64_t plane_stride,
                                      pgcn_stream_t stream) {
    const char *who = "pgcn_gatv2_softmax_f32";
    if (nrows < 0 || heads < 1 || heads > 65535 || plane_stride < 0 || nrows_wave < 0 || nrows_block < 0 || nrows_wave + nrows_block > nrows ||
        (nrows_block && !rows_block) || nrows_wave > 0x7fffffffLL * 4 || nrows_block > 0x7fffffffLL)
        return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes / row lists");
    if (nrows_wave + nrows_block == 0) return PGCN_OK;
    if (!rowptr || !E) return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (nrows_wave)
        hipLaunchKernelGGL(gatv2_softmax_kernel<64>, dim3((unsigned)((nrows_wave + kWaves - 1) / kWaves), (unsigned)heads), dim3(kThreads), 0, s,
                           rowptr, rows_wave, nrows_wave, E, plane_stride);
    if (nrows_block)
        hipLaunchKernelGGL(gatv2_softmax_kernel<256>, dim3((unsigned)nrows_block, (unsigned)heads), dim3(kThreads), 0, s, rowptr, rows_block,
                           nrows_block, E, plane_stride);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int64_t pgcn_gatv2_da_ws_elems(int64_t nrows, const int32_t *tasks, int64_t ntasks, const int64_t *seg, int32_t nslices,
                                          int32_t heads, int32_t d) {
    if (heads <= 0 || d <= 0 || nrows < 0 || ntasks < 0 || nslices < 1 || nslices > PGCN_MAX_SLICES || (nslices > 1 && (!seg || !tasks)))
        return -1;
    const int64_t grid = plan_grid(tasks != nullptr, nrows, ntasks, seg, nslices);
    return (grid + (grid + kDaGroup - 1) / kDaGroup) * heads * d;
}

extern "C" int pgcn_gatv2_grad_rows_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                                        const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const float *Zt, int64_t ldt,
                                        const float *Zs, int64_t lds, const float *a, const float *alpha, int64_t alpha_stride,
                                        const float *dOut, int64_t ldo, const float *out, int64_t ldout, float *t_ws, int32_t heads,
                                        int32_t d, float slope, float *de,
                                        int64_t de_stride, float *dZt, int64_t ldz, float *da, float *partial_ws, int64_t partial_ws_elems,
                                        int64_t nslots, float *da_ws, int64_t da_ws_elems, uint32_t flags, pgcn_stream_t stream) {
    const char *who = "pgcn_gatv2_grad_rows_f32";
    Plan pl{rowptr, col};
    int64_t grid = 0;
    const int rc = check_plan(who, heads, d, nrows, tasks, ntasks, seg, nslices, &pl, &grid);
    if (rc != PGCN_OK) return rc;
    const int64_t F = (int64_t)heads * d;
    if (ldt < F || lds < F || ldo < F || ldout < F || ldz < F || nfix < 0 || nslots < 0 || alpha_stride < 0 || de_stride < 0)
        return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes");
    if (bad_rows(Zt, ldt) || bad_rows(Zs, lds) || bad_rows(dOut, ldo) || bad_rows(out, ldout) || bad_rows(dZt, ldz) ||
        (uintptr_t)partial_ws % 16)
        return pgcn_set_error2(PGCN_EUNSUPPORTED, who, "needs 16-byte aligned operands and leading dimensions % 4 == 0");
    if (!da || !a) return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (grid == 0) {                           // no rows: da = 0
        PGCN_HIP_CHECK(hipMemsetAsync(da, 0, sizeof(float) * F, s));
        return PGCN_OK;
    }
    if (!rowptr || !col || !Zt || !Zs || !alpha || !dOut || !out || !t_ws || !de || !dZt || !da_ws || (nfix > 0 && !fix) || (nslots > 0 && !partial_ws))
        return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    const int64_t groups = (grid + kDaGroup - 1) / kDaGroup;
    if (partial_ws_elems < nslots * F || da_ws_elems < (grid + groups) * F)
        return pgcn_set_error2(PGCN_ENOMEM, who, "work-space too small (pgcn_gatv2_da_ws_elems)");
    hipLaunchKernelGGL(attn_dalpha_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, pl, Zs, lds, alpha, alpha_stride, dOut, ldo, out, ldout,
                       heads, d, (int32_t)F, de, de_stride, t_ws, partial_ws);
    PGCN_HIP_CHECK(hipGetLastError());
    if (nfix > 0) {                            // T of the cut rows, in slot order, before pass 2 takes the slots for dZt
        const int rcf = pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_ws, t_ws, heads, heads, 0, stream);
        if (rcf != PGCN_OK) return rcf;
    }
    hipLaunchKernelGGL(gatv2_grad_rows_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, pl, Zt, ldt, Zs, lds, a, alpha, alpha_stride,
                       t_ws, heads, d, (int32_t)F, slope, de, de_stride, dZt, ldz, partial_ws, flags, da_ws);
    float *stage = da_ws + grid * F;
    hipLaunchKernelGGL(gatv2_da_sum_kernel, dim3((unsigned)((groups * F + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, da_ws, grid,
                       (int64_t)kDaGroup, (int32_t)F, heads, d, stage, 0);
    hipLaunchKernelGGL(gatv2_da_sum_kernel, dim3((unsigned)((F + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, stage, groups, groups,
                       (int32_t)F, heads, d, da, 1);
    PGCN_HIP_CHECK(hipGetLastError());
    if (nfix > 0)
        return pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_ws, dZt, ldz, (int32_t)F, flags & PGCN_SPMM_ACCUMULATE, stream);
    return PGCN_OK;
}

extern "C" int pgcn_gatv2_grad_cols_f32(const int64_t *rowptr, const int32_t *col, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                                        const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const float *Zs, int64_t lds,
                                        const float *Zt, int64_t ldt, const float *dOut, int64_t ldo, const float *a, const float *alpha_t,
                                        int64_t alpha_stride, const float *de_t, int64_t de_stride, int32_t heads, int32_t d, float slope,
                                        float *dZs, int64_t ldz, float *partial_ws, int64_t partial_ws_elems, int64_t nslots, uint32_t flags,
                                        pgcn_stream_t stream) {
    const char *who = "pgcn_gatv2_grad_cols_f32";
    Plan pl{rowptr, col};
    int64_t grid = 0;
    const int rc = check_plan(who, heads, d, nrows, tasks, ntasks, seg, nslices, &pl, &grid);
    if (rc != PGCN_OK) return rc;
    const int64_t F = (int64_t)heads * d;
    if (ldt < F || lds < F || ldo < F || ldz < F || nfix < 0 || nslots < 0 || alpha_stride < 0 || de_stride < 0)
        return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes");
    if (bad_rows(Zt, ldt) || bad_rows(Zs, lds) || bad_rows(dOut, ldo) || bad_rows(dZs, ldz) || (uintptr_t)partial_ws % 16)
        return pgcn_set_error2(PGCN_EUNSUPPORTED, who, "needs 16-byte aligned operands and leading dimensions % 4 == 0");
    if (grid == 0) return PGCN_OK;
    if (!rowptr || !col || !Zs || !Zt || !dOut || !a || !alpha_t || !de_t || !dZs || (nfix > 0 && !fix) || (nslots > 0 && !partial_ws))
        return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    if (partial_ws_elems < nslots * F) return pgcn_set_error2(PGCN_ENOMEM, who, "partial work-space too small");
    hipLaunchKernelGGL(gatv2_grad_cols_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, pl, Zs, lds, Zt, ldt, dOut, ldo, a,
                       alpha_t, alpha_stride, de_t, de_stride, heads, d, (int32_t)F, slope, dZs, ldz, partial_ws, flags);
    PGCN_HIP_CHECK(hipGetLastError());
    if (nfix > 0)
        return pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_ws, dZs, ldz, (int32_t)F, flags & PGCN_SPMM_ACCUMULATE, stream);
    return PGCN_OK;
}
