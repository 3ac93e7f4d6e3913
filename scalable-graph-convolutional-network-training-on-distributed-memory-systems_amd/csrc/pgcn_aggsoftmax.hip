// pgcn_aggsoftmax.hip -- SOFTMAX aggregation over the neighbourhood (DeeperGCN, Li et al. 2020) for gfx950 (MI355X / CDNA4), fp32, and
// its backward.  One softmax PER FEATURE column c over cand(i) = the stored columns of row i (values ignored), x_j = B[j, c], beta >= 0:
//
//   LSE[i, c] = log sum_{j in cand(i)} exp(beta x_j)
//   OUT[i, c] = sum_{j in cand(i)} exp(beta x_j - LSE[i, c]) x_j                   cand(i) empty: OUT = 0.0f, LSE = -inf
//   D[j, c]   = sum_{i : j in cand(i)} G[i, c] exp(beta x_j - LSE[i, c]) (1 + beta (x_j - OUT[i, c]))     (gather form, TRANSPOSED structure)
//
// A finished pair (OUT, LSE) is a mergeable state -- "mass e^LSE with mean OUT":
//   L = max(L1, L2), e1 = exp(L1 - L), e2 = exp(L2 - L):   LSE' = L + log(e1 + e2),   OUT' = (OUT1 e1 + OUT2 e2) / (e1 + e2)
// -inf means absent; two absent groups merge to absent (no NaN).  The one rule merges the pieces of a cut row (the fix-up, in slot
// order) and implements PGCN_SPMM_ACCUMULATE (the row's current (OUT, LSE) is one more group): no third plane, no finalise pass.
//
// Mapping to the machine: the work decomposition of aggmax_tasks_kernel (pgcn_aggmax.hip) -- LPR lanes per task, VEC consecutive
// features per lane, the (col, gid) pair stream loaded coalesced and non-temporal and parked in the wave's LDS (the gid half is not
// used here, the order of the entries inside a task is free), eight row loads in flight per batch, the unsliced or the XCD-sliced plan,
// 64-feature passes.  The loads of a ragged batch are NOT predicated: the surplus slots re-read the task's last row and are selected out.
//   * forward: per element a running state (m, s, w) = (max of beta x, sum of exp(beta x - m), sum of exp(beta x - m) x) with ONE
//     transcendental per candidate:  d = beta x - m, e = exp(-|d|);  d > 0: (m, s, w) = (beta x, s e + 1, w e + x), else (s + e, w + e x).
//     The task's first candidate sets m = beta x (then d = 0, e = 1): no -inf sentinel in the loop.  OUT = w / s, LSE = m + log s.
//   * backward: row r of the transposed structure holds x = X[r, .]; per stored entry i the group loads G[i, .], OUT[i, .], LSE[i, .]
//     (three row segments) and adds G exp(beta x - LSE) (1 + beta (x - OUT)), every product and sum an explicit mul / fma so that the float4
//     body and the scalar body give the same bits.  Entries in storage order, the pieces of a cut row in slot order through
//     pgcn_spmm_fixup_f32: no atomics, deterministic.
// Inputs are finite by contract.  Plain vector loads and stores only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_device.h"
#include "pgcn_internal.h"

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kThreads = kWavesPerBlock * 64;
constexpr int kUnrollFwd = 8;   // row loads of B in flight per batch
constexpr int kUnrollBwd = 4;   // entries per batch of the backward: a row of G, of OUT and of LSE each = twelve row loads

__device__ __forceinline__ int64_t swizzle_block(int64_t b, int64_t nb, bool on) {
    if (!on) return b;
    const int64_t per = (nb + 7) / 8;   // block b runs on XCD b % 8: XCD x takes the contiguous range [x * per, (x + 1) * per)
    return (b % 8) * per + b / 8;
}

template <bool OFF32>
__device__ __forceinline__ const float *row_at(const float *base, uint32_t lane_byte_off, int32_t c, int64_t ld) {
    if constexpr (OFF32) {
        return reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + ((uint32_t)c * (uint32_t)(ld * 4) + lane_byte_off));
    } else {
        return reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + ((int64_t)c * ld * 4 + lane_byte_off));
    }
}

// the merge rule: the group (o2, l2) joins the state (o, l); l == -inf: absent
__device__ __forceinline__ void merge(float &o, float &l, float o2, float l2) {
    const float L = fmaxf(l, l2);
    if (L == -INFINITY) { o = 0.f; l = -INFINITY; return; }
    const float e1 = expf(l - L), e2 = expf(l2 - L);   // (-inf - finite = -inf: exp gives 0; one of the two is exactly 1)
    const float t = e1 + e2;
    o = (o * e1 + o2 * e2) / t;
    l = L + logf(t);
}

struct Task { int64_t kbeg; int32_t len, dst; };

struct SliceSeg { int64_t v[PGCN_MAX_SLICES + 1]; };

template <int LPR>
__device__ __forceinline__ bool my_task(int64_t ntasks, int64_t nblocks, uint32_t flags, int32_t nslices, const SliceSeg &seg,
                                        int64_t &tid, int64_t &nt) {
    constexpr int G = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    if (nslices > 1) {   // workgroup b runs on XCD b % 8 and takes tasks of slice b % nslices only
        const int slice = blockIdx.x % nslices;
        const int64_t sb = blockIdx.x / nslices;
        tid = seg.v[slice] + (sb * kWavesPerBlock + wave) * G + lane / LPR;
        nt = seg.v[slice + 1];
        return seg.v[slice] + sb * kWavesPerBlock * G < nt;
    }
    const int64_t bid = swizzle_block(blockIdx.x, nblocks, (flags & PGCN_SPMM_XCD_SWIZZLE) != 0);
    tid = (bid * kWavesPerBlock + wave) * G + lane / LPR;
    nt = ntasks;
    return bid * kWavesPerBlock * G < nt;
}

// tasks: int4 {kbeg low 32, kbeg high 32, length, dst} (pgcn_spmm_plan_host); dst >= 0: a slot, dst < 0: row ~dst.  NULL: one task per row.
__device__ __forceinline__ Task read_task(const int4 *__restrict__ tasks, const int64_t *__restrict__ rowptr, int64_t tid, bool tact) {
    Task t{0, 0, -1};
    if (tact) {
        if (tasks) {
            const int4 q = tasks[tid];
            t.kbeg = (int64_t)(((uint64_t)(uint32_t)q.y << 32) | (uint32_t)q.x);
            t.len = q.z;
            t.dst = q.w;
        } else {
            t.kbeg = rowptr[tid];
            t.len = (int32_t)(rowptr[tid + 1] - t.kbeg);
            t.dst = ~(int32_t)tid;
        }
    }
    return t;
}

// ---------------------------------------------------------------------------------------------------------------------------------
template <int LPR, int VEC, bool OFF32>
__global__ __launch_bounds__(kThreads, 6) void aggsoftmax_tasks_kernel(
    const int64_t *__restrict__ rowptr, const uint64_t *__restrict__ pairs, const int4 *__restrict__ tasks, int64_t ntasks,
    const float *__restrict__ B, int64_t ldb, float *__restrict__ OUT, int64_t ldo, float *__restrict__ LSE, int64_t ldl, float beta,
    int32_t f, float *__restrict__ pout, float *__restrict__ plse, int64_t nblocks, uint32_t flags, int32_t nslices, SliceSeg seg) {
    constexpr int U = (LPR < kUnrollFwd) ? LPR : kUnrollFwd;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int sub = lane % LPR;
    const int gbase = (lane / LPR) * LPR;

    __shared__ uint64_t meta_lds[kWavesPerBlock][64];
    uint64_t *mrow = meta_lds[wave];
    const int fcol = (blockIdx.y * LPR + sub) * VEC;   // first feature owned by this lane
    int64_t tid, nt;
    if (!my_task<LPR>(ntasks, nblocks, flags, nslices, seg, tid, nt)) return;
    const bool tact = tid < nt;
    const Task t = read_task(tasks, rowptr, tid, tact);
    const int32_t len = t.len;
    const bool fact = fcol < f;
    const uint32_t lane_off = (uint32_t)fcol * 4u;

    float m[VEC], s[VEC], w[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { m[v] = 0.f; s[v] = 0.f; w[v] = 0.f; }
    bool none = true;   // no entry of this task taken yet: the first one sets m

    // (col, gid) pairs: one per lane, streamed once -> non-temporal; the loads are unconditional (index clamped into the task; an
    // empty / inactive group reads a harmless valid word of rowptr) so that the next batch stays in flight behind the gathers
    const uint64_t *pp = (len > 0) ? pairs + t.kbeg : reinterpret_cast<const uint64_t *>(rowptr);
    const int last = (len > 0) ? len - 1 : 0;
    uint64_t np = __builtin_nontemporal_load(pp + ((sub < last) ? sub : last));
    for (int base = 0; __any(base < len); base += LPR) {
        __builtin_amdgcn_wave_barrier();
        mrow[lane] = (len > 0) ? np : 0ull;   // (an empty group gathers row 0 and keeps nothing of it)
        __builtin_amdgcn_wave_barrier();
        {
            int e = base + LPR + sub;
            e = (e < last) ? e : last;
            np = __builtin_nontemporal_load(pp + e);
        }
        const int cnt = len - base;   // entries left for this group (may be <= 0)
        const uint64_t *mg = mrow + gbase;
#pragma unroll
        for (int k = 0; k < LPR; k += U) {
            if (!__any(k < cnt)) break;
            // U independent row loads, unpredicated and back to back; in a ragged batch the surplus slots re-read the task's last
            // referenced row (the clamped pair parked above) and are kept out of the state by `ok`
            int32_t c[U];
            float x[U][VEC];
            if constexpr (U >= 2) {
#pragma unroll
                for (int u = 0; u < U; u += 2) {
                    const int4 q = *reinterpret_cast<const int4 *>(mg + k + u);   // two pairs per LDS read
                    c[u] = q.x;
                    c[u + 1] = q.z;
                }
            } else {
                c[0] = (int32_t)(uint32_t)mg[k];
            }
            if (fact) {
#pragma unroll
                for (int u = 0; u < U; ++u) vload<VEC>(x[u], row_at<OFF32>(B, lane_off, c[u], ldb));
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool ok = k + u < cnt;
                    const bool first = ok && none;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float xv = x[u][v];
                        const float bx = beta * xv;
                        const float mm = first ? bx : m[v];
                        const float d = bx - mm;
                        const float e = __expf(-fabsf(d));     // the one transcendental: the rescale of the state OR the new term
                        const bool up = ok && d > 0.f;
                        const float a = up ? e : 1.f;            // what the state is scaled by
                        const float b = ok ? (up ? 1.f : e) : 0.f;   // what the candidate weighs
                        s[v] = fmaf(s[v], a, b);
                        w[v] = fmaf(w[v], a, b * xv);
                        m[v] = up ? bx : mm;
                    }
                    none = none && !ok;
                }
            }
        }
    }

    if (tact && fact) {
        float o[VEC], l[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            o[v] = none ? 0.f : w[v] / s[v];
            l[v] = none ? -INFINITY : m[v] + logf(s[v]);
        }
        if (t.dst >= 0) {
            vstore<VEC>(pout + (int64_t)t.dst * f + fcol, o);
            vstore<VEC>(plse + (int64_t)t.dst * f + fcol, l);
        } else {
            const int64_t row = ~t.dst;
            float *po = OUT + row * ldo + fcol;
            float *pl = LSE + row * ldl + fcol;
            if (flags & PGCN_SPMM_ACCUMULATE) {   // the row's current state takes this task's result as one more group
                float oc[VEC], lc[VEC];
                vload<VEC>(oc, po);
                vload<VEC>(lc, pl);
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    merge(oc[v], lc[v], o[v], l[v]);
                    o[v] = oc[v]; l[v] = lc[v];
                }
            }
            vstore<VEC>(po, o);
            vstore<VEC>(pl, l);
        }
    }
}

// fix: int4 {row, first slot, #slots, unused}: merges the slots of a cut row in slot order
template <int LPR, int VEC>
__global__ __launch_bounds__(kThreads) void aggsoftmax_fixup_kernel(
    const int4 *__restrict__ fix, int64_t nfix, const float *__restrict__ pout, const float *__restrict__ plse,
    float *__restrict__ OUT, int64_t ldo, float *__restrict__ LSE, int64_t ldl, int32_t f, uint32_t flags) {
    constexpr int G = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t id = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * G + lane / LPR;
    const int fcol = (blockIdx.y * LPR + lane % LPR) * VEC;
    if (id >= nfix || fcol >= f) return;
    const int4 t = fix[id];
    float *po = OUT + (int64_t)t.x * ldo + fcol;
    float *pl = LSE + (int64_t)t.x * ldl + fcol;
    float o[VEC], l[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { o[v] = 0.f; l[v] = -INFINITY; }
    if (flags & PGCN_SPMM_ACCUMULATE) {
        vload<VEC>(o, po);
        vload<VEC>(l, pl);
    }
    const float *qo = pout + (int64_t)t.y * f + fcol;
    const float *ql = plse + (int64_t)t.y * f + fcol;
    for (int sl = 0; sl < t.z; ++sl) {
        float o2[VEC], l2[VEC];
        vload<VEC>(o2, qo + (int64_t)sl * f);
        vload<VEC>(l2, ql + (int64_t)sl * f);
#pragma unroll
        for (int v = 0; v < VEC; ++v) merge(o[v], l[v], o2[v], l2[v]);
    }
    vstore<VEC>(po, o);
    vstore<VEC>(pl, l);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Backward over the transposed structure: task rows are rows of D and of X, stored entries index the rows of G / OUT / LSE.
template <int LPR, int VEC, bool OFF32>
__global__ __launch_bounds__(kThreads, 4) void aggsoftmax_backward_tasks_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int4 *__restrict__ tasks, int64_t ntasks,
    const int32_t *__restrict__ slot_row, const float *__restrict__ X, int64_t ldx, const float *__restrict__ Gm, int64_t ldg,
    const float *__restrict__ OUT, int64_t ldo, const float *__restrict__ LSE, int64_t ldl, float *__restrict__ D, int64_t ldd,
    float beta, int32_t f, float *__restrict__ partial, int64_t nblocks, uint32_t flags, int32_t nslices, SliceSeg seg) {
    constexpr int U = (LPR < kUnrollBwd) ? LPR : kUnrollBwd;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int sub = lane % LPR;
    const int gbase = (lane / LPR) * LPR;

    __shared__ int32_t meta_lds[kWavesPerBlock][64];
    int32_t *mrow = meta_lds[wave];
    const int fcol = (blockIdx.y * LPR + sub) * VEC;
    int64_t tid, nt;
    if (!my_task<LPR>(ntasks, nblocks, flags, nslices, seg, tid, nt)) return;
    const bool tact = tid < nt;
    const Task t = read_task(tasks, rowptr, tid, tact);
    const int32_t len = t.len;
    const bool fact = fcol < f;
    const uint32_t lane_off = (uint32_t)fcol * 4u;

    float acc[VEC], xr[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { acc[v] = 0.f; xr[v] = 0.f; }
    if (tact && fact) {   // this task's own row of X
        const int64_t r = t.dst >= 0 ? slot_row[t.dst] : ~t.dst;
        vload<VEC>(xr, X + r * ldx + fcol);
    }

    const int32_t *cp = (len > 0) ? col + t.kbeg : reinterpret_cast<const int32_t *>(rowptr);
    const int last = (len > 0) ? len - 1 : 0;
    int32_t nc = __builtin_nontemporal_load(cp + ((sub < last) ? sub : last));
    for (int base = 0; __any(base < len); base += LPR) {
        __builtin_amdgcn_wave_barrier();
        mrow[lane] = (len > 0) ? nc : 0;
        __builtin_amdgcn_wave_barrier();
        {
            int e = base + LPR + sub;
            e = (e < last) ? e : last;
            nc = __builtin_nontemporal_load(cp + e);
        }
        const int cnt = len - base;
        const int32_t *mg = mrow + gbase;
#pragma unroll
        for (int k = 0; k < LPR; k += U) {
            if (!__any(k < cnt)) break;
            int32_t c[U];
            float g[U][VEC], o[U][VEC], l[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) c[u] = mg[k + u];
            if (fact) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    vload<VEC>(g[u], row_at<OFF32>(Gm, lane_off, c[u], ldg));
                    vload<VEC>(o[u], row_at<OFF32>(OUT, lane_off, c[u], ldo));
                    vload<VEC>(l[u], row_at<OFF32>(LSE, lane_off, c[u], ldl));
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool ok = k + u < cnt;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float p = __expf(fmaf(beta, xr[v], -l[u][v]));
                        const float q = fmaf(beta, xr[v] - o[u][v], 1.f);
                        const float gp = g[u][v] * p;
                        const float nx = fmaf(gp, q, acc[v]);
                        acc[v] = ok ? nx : acc[v];     // (a select: a surplus slot may hold inf or NaN)
                    }
                }
            }
        }
    }

    if (tact && fact) {
        if (t.dst >= 0) vstore<VEC>(partial + (int64_t)t.dst * f + fcol, acc);
        else vstore<VEC>(D + (int64_t)(~t.dst) * ldd + fcol, acc);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct Shape { int lpr, vec; };

Shape pick_shape(int32_t f, bool al16, uint32_t flags) {
    const int vec = al16 ? 4 : 1;
    const int nv = (f + vec - 1) / vec;
    int lpr = 1;
    while (lpr < nv && lpr < 64) lpr *= 2;
    if (vec == 4 && (flags & PGCN_SPMM_FPASS64) && lpr > 16) lpr = 16;   // 64 features per pass: grid y walks the passes
    return {lpr, vec};
}

bool al16(const void *p) { return (uintptr_t)p % 16 == 0; }

struct Grid { int64_t blocks, nblocks; int ntiles; };

template <int LPR, int VEC>
Grid task_grid(int64_t ntasks, int32_t f, uint32_t flags, int32_t nslices, const int64_t *seg_host, SliceSeg &seg) {
    const int64_t per_block = (int64_t)kWavesPerBlock * (64 / LPR);
    const int ntiles = (f + LPR * VEC - 1) / (LPR * VEC);
    if (nslices > 1) {   // every slice gets the blocks of the longest segment
        int64_t longest = 0;
        for (int i = 0; i <= nslices; ++i) seg.v[i] = seg_host[i];
        for (int i = 0; i < nslices; ++i)
            if (seg.v[i + 1] - seg.v[i] > longest) longest = seg.v[i + 1] - seg.v[i];
        const int64_t nb = ((longest + per_block - 1) / per_block) * nslices;
        return {nb, nb, ntiles};
    }
    const int64_t nblocks = (ntasks + per_block - 1) / per_block;
    return {(flags & PGCN_SPMM_XCD_SWIZZLE) ? ((nblocks + 7) / 8) * 8 : nblocks, nblocks, ntiles};
}

template <int LPR, int VEC>
int launch_forward(const int64_t *rowptr, const int32_t *pairs, const int32_t *tasks, int64_t ntasks, const int64_t *seg_host,
                   int32_t nslices, const int32_t *fix, int64_t nfix, const float *B, int64_t ldb, float *OUT, int64_t ldo, float *LSE,
                   int64_t ldl, float beta, int32_t f, float *pout, float *plse, uint32_t flags, hipStream_t s) {
    SliceSeg seg{};
    const Grid g = task_grid<LPR, VEC>(ntasks, f, flags, nslices, seg_host, seg);
    if (g.blocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggsoftmax_csr_plan_f32: too many tasks for one launch");
    const uint64_t *p64 = reinterpret_cast<const uint64_t *>(pairs);
    const int4 *t4 = reinterpret_cast<const int4 *>(tasks);
    if (flags & PGCN_SPMM_OFFSETS32)
        hipLaunchKernelGGL((aggsoftmax_tasks_kernel<LPR, VEC, true>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s, rowptr,
                           p64, t4, ntasks, B, ldb, OUT, ldo, LSE, ldl, beta, f, pout, plse, g.blocks, flags, nslices, seg);
    else
        hipLaunchKernelGGL((aggsoftmax_tasks_kernel<LPR, VEC, false>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s, rowptr,
                           p64, t4, ntasks, B, ldb, OUT, ldo, LSE, ldl, beta, f, pout, plse, g.blocks, flags, nslices, seg);
    PGCN_HIP_CHECK(hipGetLastError());
    if (nfix > 0) {
        const int64_t per_block = (int64_t)kWavesPerBlock * (64 / LPR);
        hipLaunchKernelGGL((aggsoftmax_fixup_kernel<LPR, VEC>), dim3((unsigned)((nfix + per_block - 1) / per_block), g.ntiles),
                           dim3(kThreads), 0, s, reinterpret_cast<const int4 *>(fix), nfix, pout, plse, OUT, ldo, LSE, ldl, f, flags);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    return PGCN_OK;
}

template <int LPR, int VEC>
int launch_backward(const int64_t *rowptr, const int32_t *col, const int32_t *tasks, int64_t ntasks, const int64_t *seg_host,
                    int32_t nslices, const int32_t *slot_row, const float *X, int64_t ldx, const float *G, int64_t ldg, const float *OUT,
                    int64_t ldo, const float *LSE, int64_t ldl, float *D, int64_t ldd, float beta, int32_t f, float *partial,
                    uint32_t flags, hipStream_t s) {
    SliceSeg seg{};
    const Grid g = task_grid<LPR, VEC>(ntasks, f, flags, nslices, seg_host, seg);
    if (g.blocks > 0x7fffffffLL)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggsoftmax_backward_csr_plan_f32: too many tasks for one launch");
    const int4 *t4 = reinterpret_cast<const int4 *>(tasks);
    if (flags & PGCN_SPMM_OFFSETS32)
        hipLaunchKernelGGL((aggsoftmax_backward_tasks_kernel<LPR, VEC, true>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s,
                           rowptr, col, t4, ntasks, slot_row, X, ldx, G, ldg, OUT, ldo, LSE, ldl, D, ldd, beta, f, partial, g.blocks,
                           flags, nslices, seg);
    else
        hipLaunchKernelGGL((aggsoftmax_backward_tasks_kernel<LPR, VEC, false>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s,
                           rowptr, col, t4, ntasks, slot_row, X, ldx, G, ldg, OUT, ldo, LSE, ldl, D, ldd, beta, f, partial, g.blocks,
                           flags, nslices, seg);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

bool bad_beta(float beta) { return !(beta >= 0.f) || isinf(beta); }   // (NaN fails the comparison)

}  // namespace

#define PGCN_AGGSOFTMAX_SHAPES(CASE)                                                       \
    CASE(1, 4) CASE(2, 4) CASE(4, 4) CASE(8, 4) CASE(16, 4) CASE(32, 4) CASE(64, 4)        \
    CASE(1, 1) CASE(2, 1) CASE(4, 1) CASE(8, 1) CASE(16, 1) CASE(32, 1) CASE(64, 1)

extern "C" int pgcn_aggsoftmax_csr_plan_f32(const int64_t *rowptr, const int32_t *pairs, const int32_t *tasks, int64_t ntasks,
                                            const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const float *B,
                                            int64_t ldb, float *OUT, int64_t ldo, float *LSE, int64_t ldl, float beta, int32_t f,
                                            void *ws, int64_t ws_bytes, int64_t nslots, uint32_t flags, pgcn_stream_t stream) {
    if (ntasks < 0 || nfix < 0 || nslots < 0 || f < 1 || ldb < f || ldo < f || ldl < f || nslices < 1 || nslices > PGCN_MAX_SLICES ||
        (nslices > 1 && (!seg || !tasks)) || bad_beta(beta))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggsoftmax_csr_plan_f32: bad sizes");
    if (nslices > 1 && (seg[0] != 0 || seg[nslices] != ntasks))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggsoftmax_csr_plan_f32: seg does not cover the task list");
    if (ntasks == 0) return PGCN_OK;
    if (!rowptr || !pairs || !B || !OUT || !LSE || (nfix > 0 && (!fix || !tasks)) || (nslots > 0 && !ws))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggsoftmax_csr_plan_f32: null pointer");
    if (ntasks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggsoftmax_csr_plan_f32: ntasks >= 2^31");
    if ((uintptr_t)pairs % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggsoftmax_csr_plan_f32: pairs must be 8-byte aligned");
    if (ws_bytes < nslots * (int64_t)f * 8)
        return pgcn_set_error(PGCN_ENOMEM, "pgcn_aggsoftmax_csr_plan_f32: work-space too small");
    float *pout = reinterpret_cast<float *>(ws);                 // OUT plane, then LSE plane: nslots x f each
    float *plse = reinterpret_cast<float *>(ws) + nslots * (int64_t)f;
    const Shape sh = pick_shape(f, al16(B) && al16(OUT) && al16(LSE) && al16(pout) && al16(plse) && ldb % 4 == 0 && ldo % 4 == 0 &&
                                       ldl % 4 == 0 && f % 4 == 0, flags);
#define PGCN_CASE(L, V)                                                                                                              \
    if (sh.lpr == L && sh.vec == V)                                                                                                  \
        return launch_forward<L, V>(rowptr, pairs, tasks, ntasks, seg, nslices, fix, nfix, B, ldb, OUT, ldo, LSE, ldl, beta, f, pout, \
                                    plse, flags, (hipStream_t)stream);
    PGCN_AGGSOFTMAX_SHAPES(PGCN_CASE)
#undef PGCN_CASE
    return pgcn_set_error(PGCN_EINVAL, "pgcn_aggsoftmax_csr_plan_f32: no kernel shape");
}

extern "C" int pgcn_aggsoftmax_backward_csr_plan_f32(const int64_t *rowptr, const int32_t *col, const int32_t *slot_row,
                                                     const int32_t *tasks, int64_t ntasks, const int64_t *seg, int32_t nslices,
                                                     const int32_t *fix, int64_t nfix, const float *X, int64_t ldx, const float *G,
                                                     int64_t ldg, const float *OUT, int64_t ldo, const float *LSE, int64_t ldl, float *D,
                                                     int64_t ldd, float beta, int32_t f, float *partial_ws, int64_t partial_ws_elems,
                                                     int64_t nslots, uint32_t flags, pgcn_stream_t stream) {
    if (ntasks < 0 || nfix < 0 || nslots < 0 || f < 1 || ldx < f || ldg < f || ldo < f || ldl < f || ldd < f || nslices < 1 ||
        nslices > PGCN_MAX_SLICES || (nslices > 1 && (!seg || !tasks)) || bad_beta(beta))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggsoftmax_backward_csr_plan_f32: bad sizes");
    if (nslices > 1 && (seg[0] != 0 || seg[nslices] != ntasks))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggsoftmax_backward_csr_plan_f32: seg does not cover the task list");
    if (ntasks == 0) return PGCN_OK;
    if (!rowptr || !col || !X || !G || !OUT || !LSE || !D || (nfix > 0 && (!fix || !tasks)) || (nslots > 0 && (!partial_ws || !slot_row)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggsoftmax_backward_csr_plan_f32: null pointer");
    if (ntasks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggsoftmax_backward_csr_plan_f32: ntasks >= 2^31");
    if (partial_ws_elems < nslots * (int64_t)f)
        return pgcn_set_error(PGCN_ENOMEM, "pgcn_aggsoftmax_backward_csr_plan_f32: partial work-space too small");
    const Shape sh = pick_shape(f, al16(X) && al16(G) && al16(OUT) && al16(LSE) && al16(D) && al16(partial_ws) && ldx % 4 == 0 &&
                                       ldg % 4 == 0 && ldo % 4 == 0 && ldl % 4 == 0 && ldd % 4 == 0 && f % 4 == 0, flags);
    int rc = 1;   // (no shape taken yet)
#define PGCN_CASE(L, V)                                                                                                              \
    if (sh.lpr == L && sh.vec == V)                                                                                                  \
        rc = launch_backward<L, V>(rowptr, col, tasks, ntasks, seg, nslices, slot_row, X, ldx, G, ldg, OUT, ldo, LSE, ldl, D, ldd, beta, \
                                   f, partial_ws, flags, (hipStream_t)stream);
    PGCN_AGGSOFTMAX_SHAPES(PGCN_CASE)
#undef PGCN_CASE
    if (rc == 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggsoftmax_backward_csr_plan_f32: no kernel shape");
    if (rc != PGCN_OK || nfix == 0) return rc;
    // the pieces of a cut row, added in slot order (the sum path's fix-up: the slots hold plain partial sums)
    return pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_ws, D, ldd, f, 0u, stream);
}
