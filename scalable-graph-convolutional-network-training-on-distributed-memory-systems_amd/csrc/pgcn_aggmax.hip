// pgcn_aggmax.hip -- element-wise MAX over the neighbourhood for gfx950 (MI355X / CDNA4), fp32, and its backward.
//
//   OUT[i, c] = max_{j in cand(i)} B[j, c]          cand(i) = the stored columns of row i (values ignored)
//   ARG[i, c] = the SMALLEST GLOBAL id of a j that attains it (fp32 ==: -0.0 ties with +0.0; OUT takes that j's bits)
//   cand(i) empty: OUT = 0.0f, ARG = -1
//   D[j, c]   = sum over { i : ARG[i, c] == gid(j) } of G[i, c]      (gather form over the TRANSPOSED structure)
//
// The tie-break is a total order on global ids, so (OUT, ARG) depend neither on the local numbering, nor on the split of a row's
// candidates over several launches (local block, then the halo blocks with PGCN_SPMM_ACCUMULATE), nor on the cut of a long row into
// tasks: a candidate (v, g) replaces the state (cur, a) when  a < 0 || v > cur || (v == cur && g < a)  -- no -inf sentinel, every
// launch that does not accumulate starts every row at (0.0f, -1).  Inputs are finite by contract.
//
// Mapping to the machine: the work decomposition of spmm_tasks_kernel (pgcn_spmm.hip) -- a group of LPR lanes owns one task (a row, or
// one <= chunk piece of a long row), a lane owns VEC consecutive features so that a group reads a row of B as one coalesced segment,
// the index stream is loaded coalesced and non-temporal and parked in the wave's LDS, eight row loads are in flight per batch.
//   * forward: the stream holds PAIRS (col, global id of col): the 8 bytes per entry the sum path spends on (col, val), so the
//     tie-break costs no extra gather.  Per feature a lane keeps (cur, arg) and updates it with compares and selects: no branch on data.
//     The pairs of every TASK are stored in ASCENDING GLOBAL ID (kernels.prepare_max: a row that is one task is ordered as a whole, a
//     sliced row per col % nslices group; it checks the structure against the plan), so inside a task an equal value never replaces: the rule shrinks to `first entry || v > cur` -- one compare and two selects per element
//     (the full rule is ~7 VALU operations per element and made the kernel VALU-bound: 14.7 G elements on the benchmark graph).  The
//     full rule merges tasks: slots in the fix-up, the row's current state under PGCN_SPMM_ACCUMULATE.
//   * pieces of a cut row write (value, arg) to a value plane and an arg plane of the caller's work-space; aggmax_fixup_kernel merges the
//     slots in slot order with the same rule (any order gives the same bits).
//   * backward: row r of the transposed structure has global id rowgid[r]; for every stored entry i the group loads G[i, .] and
//     ARG[i, .] (two row segments) and adds ARG == rowgid[r] ? G : 0.  No atomics; entries in storage order, the pieces of a cut row in
//     slot order through pgcn_spmm_fixup_f32: deterministic.
//   * plans: the unsliced plan (XCD swizzle: one contiguous row range per XCD), or the XCD-sliced plan of the sum path -- the entries of a
//     row stored grouped by col % nslices, task segment s run by the workgroups with blockIdx.x % nslices == s, which the dispatcher places
//     on XCD s: every private 4 MiB L2 then caches a disjoint 1 / nslices of the rows of B (of G and ARG backward).  Placement and the
//     cut of the rows only: the forward's bits do not depend on them.  PGCN_SPMM_FPASS64: 64 features per pass (grid y, pass-major).
// A float4 / int4 body when f, the leading dimensions and the pointers allow it, a guarded scalar body otherwise: the same bits (the
// forward does no arithmetic, the backward adds in the same order).  Plain vector loads and stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgcn_device.h"
#include "pgcn_internal.h"

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kThreads = kWavesPerBlock * 64;
constexpr int kUnrollFwd = 8;   // row loads of B in flight per batch
constexpr int kUnrollBwd = 4;   // entries per batch of the backward: a row of G and a row of ARG each = eight row loads

__device__ __forceinline__ int64_t swizzle_block(int64_t b, int64_t nb, bool on) {
    if (!on) return b;
    const int64_t per = (nb + 7) / 8;   // block b runs on XCD b % 8: XCD x takes the contiguous range [x * per, (x + 1) * per)
    return (b % 8) * per + b / 8;
}

template <int VEC>
__device__ __forceinline__ void iload(int32_t (&x)[VEC], const int32_t *p) {
    if constexpr (VEC == 1) { x[0] = *p; }
    if constexpr (VEC == 4) {
        const int4 v = *reinterpret_cast<const int4 *>(p);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    }
}

template <int VEC>
__device__ __forceinline__ void istore(int32_t *p, const int32_t (&x)[VEC]) {
    if constexpr (VEC == 1) { *p = x[0]; }
    if constexpr (VEC == 4) { *reinterpret_cast<int4 *>(p) = make_int4(x[0], x[1], x[2], x[3]); }
}

// Address of (row c, this lane's first feature) of a row-major 4-byte matrix.  OFF32: the caller guarantees that every byte offset
// fits 32 bits -- a uniform 64-bit base plus a 32-bit lane offset instead of a 64-bit multiply-add per load.
template <bool OFF32>
__device__ __forceinline__ const void *row_at(const void *base, uint32_t lane_byte_off, int32_t c, int64_t ld) {
    if constexpr (OFF32) {
        return reinterpret_cast<const char *>(base) + ((uint32_t)c * (uint32_t)(ld * 4) + lane_byte_off);
    } else {
        return reinterpret_cast<const char *>(base) + ((int64_t)c * ld * 4 + lane_byte_off);
    }
}

// the update rule; `ok`: the candidate exists (an entry inside the task / a slot or a row that holds an arg)
__device__ __forceinline__ void take_max(float &cur, int32_t &arg, float v, int32_t g, bool ok) {
    const bool take = ok && (arg < 0 || v > cur || (v == cur && g < arg));
    cur = take ? v : cur;
    arg = take ? g : arg;
}

struct Task { int64_t kbeg; int32_t len, dst; };

struct SliceSeg { int64_t v[PGCN_MAX_SLICES + 1]; };

// The task of this group of LPR lanes: (task id, one past the last id it may take), or false when the whole workgroup has none.
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
__global__ __launch_bounds__(kThreads, 6) void aggmax_tasks_kernel(
    const int64_t *__restrict__ rowptr, const uint64_t *__restrict__ pairs, const int4 *__restrict__ tasks, int64_t ntasks,
    const float *__restrict__ B, int64_t ldb, float *__restrict__ OUT, int64_t ldo, int32_t *__restrict__ ARG, int64_t lda,
    int32_t f, float *__restrict__ pval, int32_t *__restrict__ parg, int64_t nblocks, uint32_t flags, int32_t nslices, SliceSeg seg) {
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

    float cur[VEC];
    int32_t arg[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { cur[v] = 0.f; arg[v] = -1; }
    bool none = true;   // no entry of this task taken yet (the first one is taken for every feature: arg < 0 for all of them or none)

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
            int32_t c[U], g[U];
            float x[U][VEC];
            if constexpr (U >= 2) {
#pragma unroll
                for (int u = 0; u < U; u += 2) {
                    const int4 m = *reinterpret_cast<const int4 *>(mg + k + u);   // two pairs per LDS read
                    c[u] = m.x; g[u] = m.y;
                    c[u + 1] = m.z; g[u + 1] = m.w;
                }
            } else {
                const uint64_t m = mg[k];
                c[0] = (int32_t)(uint32_t)m; g[0] = (int32_t)(uint32_t)(m >> 32);
            }
            if (fact) {
#pragma unroll
                for (int u = 0; u < U; ++u) vload<VEC>(x[u], reinterpret_cast<const float *>(row_at<OFF32>(B, lane_off, c[u], ldb)));
#pragma unroll
                for (int u = 0; u < U; ++u) {   // ascending global ids inside a task: an equal value never replaces
                    const bool ok = k + u < cnt;
                    const bool first = ok && none;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const bool take = first || (ok && x[u][v] > cur[v]);
                        cur[v] = take ? x[u][v] : cur[v];
                        arg[v] = take ? g[u] : arg[v];
                    }
                    none = none && !ok;
                }
            }
        }
    }

    if (tact && fact) {
        if (t.dst >= 0) {
            vstore<VEC>(pval + (int64_t)t.dst * f + fcol, cur);
            istore<VEC>(parg + (int64_t)t.dst * f + fcol, arg);
        } else {
            const int64_t row = ~t.dst;
            float *o = OUT + row * ldo + fcol;
            int32_t *a = ARG + row * lda + fcol;
            if (flags & PGCN_SPMM_ACCUMULATE) {   // the row's current state takes this task's result as one more candidate
                float oc[VEC];
                int32_t oa[VEC];
                vload<VEC>(oc, o);
                iload<VEC>(oa, a);
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    take_max(oc[v], oa[v], cur[v], arg[v], arg[v] >= 0);
                    cur[v] = oc[v]; arg[v] = oa[v];
                }
            }
            vstore<VEC>(o, cur);
            istore<VEC>(a, arg);
        }
    }
}

// fix: int4 {row, first slot, #slots, unused}: merges the slots of a cut row in slot order
template <int LPR, int VEC>
__global__ __launch_bounds__(kThreads) void aggmax_fixup_kernel(
    const int4 *__restrict__ fix, int64_t nfix, const float *__restrict__ pval, const int32_t *__restrict__ parg,
    float *__restrict__ OUT, int64_t ldo, int32_t *__restrict__ ARG, int64_t lda, int32_t f, uint32_t flags) {
    constexpr int G = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t id = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * G + lane / LPR;
    const int fcol = (blockIdx.y * LPR + lane % LPR) * VEC;
    if (id >= nfix || fcol >= f) return;
    const int4 t = fix[id];
    float *o = OUT + (int64_t)t.x * ldo + fcol;
    int32_t *a = ARG + (int64_t)t.x * lda + fcol;
    float cur[VEC];
    int32_t arg[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { cur[v] = 0.f; arg[v] = -1; }
    if (flags & PGCN_SPMM_ACCUMULATE) {
        vload<VEC>(cur, o);
        iload<VEC>(arg, a);
    }
    const float *pv = pval + (int64_t)t.y * f + fcol;
    const int32_t *pa = parg + (int64_t)t.y * f + fcol;
    int s = 0;
    for (; s + 4 <= t.z; s += 4) {   // four slots in flight, merged in slot order
        float x[4][VEC];
        int32_t g[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            vload<VEC>(x[u], pv + (int64_t)(s + u) * f);
            iload<VEC>(g[u], pa + (int64_t)(s + u) * f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < VEC; ++v) take_max(cur[v], arg[v], x[u][v], g[u][v], g[u][v] >= 0);
    }
    for (; s < t.z; ++s) {
        float x[VEC];
        int32_t g[VEC];
        vload<VEC>(x, pv + (int64_t)s * f);
        iload<VEC>(g, pa + (int64_t)s * f);
#pragma unroll
        for (int v = 0; v < VEC; ++v) take_max(cur[v], arg[v], x[v], g[v], g[v] >= 0);
    }
    vstore<VEC>(o, cur);
    istore<VEC>(a, arg);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Backward over the transposed structure: task rows are rows of D, stored entries index the rows of G / ARG.
template <int LPR, int VEC, bool OFF32>
__global__ __launch_bounds__(kThreads, 6) void aggmax_backward_tasks_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int4 *__restrict__ tasks, int64_t ntasks,
    const int32_t *__restrict__ rowgid, const int32_t *__restrict__ slot_row, const float *__restrict__ Gm, int64_t ldg,
    const int32_t *__restrict__ ARG, int64_t lda, float *__restrict__ D, int64_t ldd, int32_t f, float *__restrict__ partial,
    int64_t nblocks, uint32_t flags, int32_t nslices, SliceSeg seg) {
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
    // the global id this task's row answers to (-2: no task; ARG holds ids >= 0 or -1, so nothing matches)
    const int32_t gid = tact ? rowgid[t.dst >= 0 ? slot_row[t.dst] : ~t.dst] : -2;

    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;

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
            float x[U][VEC];
            int32_t a[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) c[u] = mg[k + u];
            if (fact) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    vload<VEC>(x[u], reinterpret_cast<const float *>(row_at<OFF32>(Gm, lane_off, c[u], ldg)));
                    iload<VEC>(a[u], reinterpret_cast<const int32_t *>(row_at<OFF32>(ARG, lane_off, c[u], lda)));
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool ok = k + u < cnt;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] += (ok && a[u][v] == gid) ? x[u][v] : 0.f;
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
                   int32_t nslices, const int32_t *fix,
                   int64_t nfix, const float *B, int64_t ldb, float *OUT, int64_t ldo, int32_t *ARG, int64_t lda, int32_t f,
                   float *pval, int32_t *parg, uint32_t flags, hipStream_t s) {
    SliceSeg seg{};
    const Grid g = task_grid<LPR, VEC>(ntasks, f, flags, nslices, seg_host, seg);
    if (g.blocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggmax_csr_plan_f32: too many tasks for one launch");
    const uint64_t *p64 = reinterpret_cast<const uint64_t *>(pairs);
    const int4 *t4 = reinterpret_cast<const int4 *>(tasks);
    if (flags & PGCN_SPMM_OFFSETS32)
        hipLaunchKernelGGL((aggmax_tasks_kernel<LPR, VEC, true>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s, rowptr, p64,
                           t4, ntasks, B, ldb, OUT, ldo, ARG, lda, f, pval, parg, g.blocks, flags, nslices, seg);
    else
        hipLaunchKernelGGL((aggmax_tasks_kernel<LPR, VEC, false>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s, rowptr, p64,
                           t4, ntasks, B, ldb, OUT, ldo, ARG, lda, f, pval, parg, g.blocks, flags, nslices, seg);
    PGCN_HIP_CHECK(hipGetLastError());
    if (nfix > 0) {
        const int64_t per_block = (int64_t)kWavesPerBlock * (64 / LPR);
        hipLaunchKernelGGL((aggmax_fixup_kernel<LPR, VEC>), dim3((unsigned)((nfix + per_block - 1) / per_block), g.ntiles),
                           dim3(kThreads), 0, s, reinterpret_cast<const int4 *>(fix), nfix, pval, parg, OUT, ldo, ARG, lda, f, flags);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    return PGCN_OK;
}

template <int LPR, int VEC>
int launch_backward(const int64_t *rowptr, const int32_t *col, const int32_t *tasks, int64_t ntasks, const int64_t *seg_host,
                    int32_t nslices, const int32_t *rowgid,
                    const int32_t *slot_row, const float *G, int64_t ldg, const int32_t *ARG, int64_t lda, float *D, int64_t ldd,
                    int32_t f, float *partial, uint32_t flags, hipStream_t s) {
    SliceSeg seg{};
    const Grid g = task_grid<LPR, VEC>(ntasks, f, flags, nslices, seg_host, seg);
    if (g.blocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggmax_backward_csr_plan_f32: too many tasks for one launch");
    const int4 *t4 = reinterpret_cast<const int4 *>(tasks);
    if (flags & PGCN_SPMM_OFFSETS32)
        hipLaunchKernelGGL((aggmax_backward_tasks_kernel<LPR, VEC, true>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s,
                           rowptr, col, t4, ntasks, rowgid, slot_row, G, ldg, ARG, lda, D, ldd, f, partial, g.blocks, flags, nslices, seg);
    else
        hipLaunchKernelGGL((aggmax_backward_tasks_kernel<LPR, VEC, false>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s,
                           rowptr, col, t4, ntasks, rowgid, slot_row, G, ldg, ARG, lda, D, ldd, f, partial, g.blocks, flags, nslices, seg);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

}  // namespace

#define PGCN_AGGMAX_SHAPES(CASE)                                                           \
    CASE(1, 4) CASE(2, 4) CASE(4, 4) CASE(8, 4) CASE(16, 4) CASE(32, 4) CASE(64, 4)        \
    CASE(1, 1) CASE(2, 1) CASE(4, 1) CASE(8, 1) CASE(16, 1) CASE(32, 1) CASE(64, 1)

extern "C" int pgcn_aggmax_csr_plan_f32(const int64_t *rowptr, const int32_t *pairs, const int32_t *tasks, int64_t ntasks,
                                        const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const float *B, int64_t ldb, float *OUT, int64_t ldo,
                                        int32_t *ARG, int64_t lda, int32_t f, void *ws, int64_t ws_bytes, int64_t nslots,
                                        uint32_t flags, pgcn_stream_t stream) {
    if (ntasks < 0 || nfix < 0 || nslots < 0 || f < 1 || ldb < f || ldo < f || lda < f || nslices < 1 || nslices > PGCN_MAX_SLICES ||
        (nslices > 1 && (!seg || !tasks)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggmax_csr_plan_f32: bad sizes");
    if (nslices > 1 && (seg[0] != 0 || seg[nslices] != ntasks))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggmax_csr_plan_f32: seg does not cover the task list");
    if (ntasks == 0) return PGCN_OK;
    if (!rowptr || !pairs || !B || !OUT || !ARG || (nfix > 0 && (!fix || !tasks)) || (nslots > 0 && !ws))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggmax_csr_plan_f32: null pointer");
    if (ntasks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggmax_csr_plan_f32: ntasks >= 2^31");
    if ((uintptr_t)pairs % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggmax_csr_plan_f32: pairs must be 8-byte aligned");
    if (ws_bytes < nslots * (int64_t)f * 8)
        return pgcn_set_error(PGCN_ENOMEM, "pgcn_aggmax_csr_plan_f32: work-space too small");
    float *pval = reinterpret_cast<float *>(ws);                 // value plane, then arg plane: nslots x f each
    int32_t *parg = reinterpret_cast<int32_t *>(ws) + nslots * (int64_t)f;
    const Shape sh = pick_shape(f, al16(B) && al16(OUT) && al16(ARG) && al16(pval) && al16(parg) && ldb % 4 == 0 && ldo % 4 == 0 &&
                                       lda % 4 == 0 && f % 4 == 0, flags);
#define PGCN_CASE(L, V)                                                                                                       \
    if (sh.lpr == L && sh.vec == V)                                                                                           \
        return launch_forward<L, V>(rowptr, pairs, tasks, ntasks, seg, nslices, fix, nfix, B, ldb, OUT, ldo, ARG, lda, f, pval, \
                                    parg, flags, (hipStream_t)stream);
    PGCN_AGGMAX_SHAPES(PGCN_CASE)
#undef PGCN_CASE
    return pgcn_set_error(PGCN_EINVAL, "pgcn_aggmax_csr_plan_f32: no kernel shape");
}

extern "C" int pgcn_aggmax_backward_csr_plan_f32(const int64_t *rowptr, const int32_t *col, const int32_t *rowgid,
                                                 const int32_t *slot_row, const int32_t *tasks, int64_t ntasks, const int64_t *seg,
                                                 int32_t nslices, const int32_t *fix,
                                                 int64_t nfix, const float *G, int64_t ldg, const int32_t *ARG, int64_t lda, float *D,
                                                 int64_t ldd, int32_t f, float *partial_ws, int64_t partial_ws_elems, int64_t nslots,
                                                 uint32_t flags, pgcn_stream_t stream) {
    if (ntasks < 0 || nfix < 0 || nslots < 0 || f < 1 || ldg < f || lda < f || ldd < f || nslices < 1 || nslices > PGCN_MAX_SLICES ||
        (nslices > 1 && (!seg || !tasks)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggmax_backward_csr_plan_f32: bad sizes");
    if (nslices > 1 && (seg[0] != 0 || seg[nslices] != ntasks))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggmax_backward_csr_plan_f32: seg does not cover the task list");
    if (ntasks == 0) return PGCN_OK;
    if (!rowptr || !col || !rowgid || !G || !ARG || !D || (nfix > 0 && (!fix || !tasks)) || (nslots > 0 && (!partial_ws || !slot_row)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggmax_backward_csr_plan_f32: null pointer");
    if (ntasks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggmax_backward_csr_plan_f32: ntasks >= 2^31");
    if (partial_ws_elems < nslots * (int64_t)f)
        return pgcn_set_error(PGCN_ENOMEM, "pgcn_aggmax_backward_csr_plan_f32: partial work-space too small");
    const Shape sh = pick_shape(f, al16(G) && al16(ARG) && al16(D) && al16(partial_ws) && ldg % 4 == 0 && lda % 4 == 0 && ldd % 4 == 0 &&
                                       f % 4 == 0, flags);
    int rc = 1;   // (no shape taken yet)
#define PGCN_CASE(L, V)                                                                                                          \
    if (sh.lpr == L && sh.vec == V)                                                                                                \
        rc = launch_backward<L, V>(rowptr, col, tasks, ntasks, seg, nslices, rowgid, slot_row, G, ldg, ARG, lda, D, ldd, f, partial_ws, \
                                   flags, (hipStream_t)stream);
    PGCN_AGGMAX_SHAPES(PGCN_CASE)
#undef PGCN_CASE
    if (rc == 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggmax_backward_csr_plan_f32: no kernel shape");
    if (rc != PGCN_OK || nfix == 0) return rc;
    // the pieces of a cut row, added in slot order (the sum path's fix-up: the slots hold plain partial sums)
    return pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_ws, D, ldd, f, 0u, stream);
}
