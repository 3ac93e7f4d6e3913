// pgcn_dropedge.hip -- DropEdge for gfx950 (MI355X / CDNA4): the aggregation over a pattern whose entries are dropped anew at every
// training step (Rong et al., ICLR 2020), fp32.  include/pgcn_hip.h has the contract, pgcn_dropedge.h the keep function.
//
//   keep(gi, gj) = gi == gj || u(seed, step, min, max) >= thr        (GLOBAL ids: symmetric, partition-independent, self loops stay)
//   sum     C[i, .] (+)= sum over the KEPT stored entries (i, j) of B[j, .]             pgcn_dropedge_sum_csr_plan_f32
//   count   n[i]    (+)= number of kept stored entries of row i (exact int32)            pgcn_dropedge_count_csr_plan_i32
//   scales  s[i] = n[i] > 0 ? fl32(1 / sqrt((double)n[i])) : 1                           pgcn_dropedge_scales_f32
//   scale   Y[i, .] = fl(s[i] * X[i, .])                                                 pgcn_row_scale_f32
// The renormalised dropped matrix D_r^-1/2 M D_c^-1/2 is then scale . sum . scale: no value array, nothing rebuilt on the host.
//
// Mapping to the machine.  The sum kernel is the forward of pgcn_aggmax.hip with another update: a group of LPR lanes owns one task
// (a row, or one <= chunk piece of a long row), a lane owns VEC consecutive features, the (col, global id) pair stream is loaded
// coalesced and non-temporal, eight row loads are in flight per batch, the unsliced or the XCD-sliced plan, 64-feature passes.
//   * keep is evaluated ONCE per entry, by the lane that loaded the pair: two 32-bit mixes.  The kept columns of a batch are
//     COMPACTED into the wave's LDS (a ballot and two population counts give every kept entry its place in its group's list), so a
//     dropped entry costs the gather nothing: no row load, no slot of a batch of loads, no multiply by zero -- whatever its row
//     holds.  The loads stay unpredicated (a predicated load made the compiler wait for each one at the join): the places behind
//     the kept ones of a ragged batch re-read the group's last kept row, as the max kernel's surplus slots do, and a select keeps
//     them out of the sum.  The gather kernels are bound by row loads that miss L2: at p = 0.5 half are gone.
//   * the kept entries are added in storage order; the pieces of a cut row go through pgcn_spmm_fixup_f32 in slot order:
//     deterministic, no float atomics.  A float4 body and a guarded scalar body add in the same order: the same bits.
//   * the step is read from DEVICE memory: a new step needs no rebinding, a captured graph draws a new mask at every replay.
// The count kernel walks the same plan and pair stream with 16 lanes per task and loads no rows; the pieces of a cut row are added
// with integer atomics (exact in any order) after the counts were zeroed.  This file is compiled with -ffp-contract=off
// (csrc/build.sh); the row scale is one rounded product per element in the layout of pgcn_rowband.h.  Plain vector loads and stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_device.h"
#include "pgcn_internal.h"
#include "pgcn_rowband.h"
#include "pgcn_dropedge.h"

namespace {

constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 8;        // row loads of B in flight per batch
constexpr int kCountLanes = 16;   // lanes per task of the count kernel: 128 contiguous bytes of pairs per step
constexpr int kRowsInFlight = 4;  // rows per thread of the row scale

__device__ __forceinline__ int64_t swizzle_block(int64_t b, int64_t nb, bool on) {
    if (!on) return b;
    const int64_t per = (nb + 7) / 8;   // block b runs on XCD b % 8: XCD x takes the contiguous range [x * per, (x + 1) * per)
    return (b % 8) * per + b / 8;
}

// Address of (row c, this lane's first feature) of a row-major fp32 matrix.  OFF32: every byte offset fits 32 bits.
template <bool OFF32>
__device__ __forceinline__ const float *row_at(const float *base, uint32_t lane_byte_off, int32_t c, int64_t ld) {
    if constexpr (OFF32) {
        return reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + ((uint32_t)c * (uint32_t)(ld * 4) + lane_byte_off));
    } else {
        return reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + ((int64_t)c * ld * 4 + lane_byte_off));
    }
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
        tid = seg.v[slice] + (sb * kWaves + wave) * G + lane / LPR;
        nt = seg.v[slice + 1];
        return seg.v[slice] + sb * kWaves * G < nt;
    }
    const int64_t bid = swizzle_block(blockIdx.x, nblocks, (flags & PGCN_SPMM_XCD_SWIZZLE) != 0);
    tid = (bid * kWaves + wave) * G + lane / LPR;
    nt = ntasks;
    return bid * kWaves * G < nt;
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

// the global id of the row a task belongs to (an inactive group: 0, it keeps nothing)
__device__ __forceinline__ uint32_t task_gid(const Task &t, bool tact, const int32_t *__restrict__ rowgid, const int32_t *__restrict__ slot_row) {
    return tact ? (uint32_t)rowgid[t.dst >= 0 ? slot_row[t.dst] : ~t.dst] : 0u;
}

// ---------------------------------------------------------------------------------------------------------------------------------
template <int LPR, int VEC, bool OFF32>
__global__ __launch_bounds__(kThreads, 6) void dropedge_sum_kernel(
    const int64_t *__restrict__ rowptr, const uint64_t *__restrict__ pairs, const int4 *__restrict__ tasks, int64_t ntasks,
    const int32_t *__restrict__ rowgid, const int32_t *__restrict__ slot_row, const float *__restrict__ B, int64_t ldb,
    float *__restrict__ C, int64_t ldc, int32_t f, float *__restrict__ partial, int64_t nblocks, uint32_t flags, int32_t nslices,
    SliceSeg seg, uint64_t seed, const int64_t *__restrict__ step, uint32_t thr) {
    constexpr int U = (LPR < kUnroll) ? LPR : kUnroll;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int sub = lane % LPR;
    const int gbase = (lane / LPR) * LPR;

    __shared__ __attribute__((aligned(16))) int32_t meta_lds[kWaves][64];
    int32_t *mrow = meta_lds[wave];
    const int fcol = (blockIdx.y * LPR + sub) * VEC;   // first feature owned by this lane
    int64_t tid, nt;
    if (!my_task<LPR>(ntasks, nblocks, flags, nslices, seg, tid, nt)) return;
    const bool tact = tid < nt;
    const Task t = read_task(tasks, rowptr, tid, tact);
    const int32_t len = t.len;
    const bool fact = fcol < f;
    const uint32_t lane_off = (uint32_t)fcol * 4u;
    const uint32_t gi = task_gid(t, tact, rowgid, slot_row);
    const uint64_t key = dropedge_key(seed, (uint64_t)step[0]);
    const uint64_t gmask = (LPR == 64) ? ~0ull : (((1ull << (LPR & 63)) - 1ull) << gbase);   // the lanes of this group
    const uint64_t below = (1ull << lane) - 1ull;

    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;

    // (col, gid) pairs: one per lane, streamed once -> non-temporal; the loads are unconditional (index clamped into the task; an
    // empty / inactive group reads a harmless valid word of rowptr) so that the next batch stays in flight behind the gathers
    const uint64_t *pp = (len > 0) ? pairs + t.kbeg : reinterpret_cast<const uint64_t *>(rowptr);
    const int last = (len > 0) ? len - 1 : 0;
    uint64_t np = __builtin_nontemporal_load(pp + ((sub < last) ? sub : last));
    int32_t safe = 0;   // what a list place without a kept entry gathers: a valid row in any case (a wave with an entry has a row 0 of B)
    for (int base = 0; __any(base < len); base += LPR) {
        // this lane's entry: hashed once, here; the kept columns of the group's batch are compacted to the front of its LDS list
        const int32_t mycol = (int32_t)(uint32_t)np;
        const bool kp = (base + sub < len) && dropedge_keep(key, gi, (uint32_t)(np >> 32), thr);
        const uint64_t bal = __ballot(kp) & gmask;
        const int kcnt = __popcll(bal);                // kept entries of this group's batch (the same in every lane of the group)
        const int pos = __popcll(bal & below);         // kept lanes of the group below this one
        // the places behind the kept ones take the group's LAST KEPT column (of this batch, else of an earlier one, else row 0 of B):
        // a row the group has just read, so that every load below is issued unconditionally and nothing waits on a branch
        const int32_t lastcol = __shfl(mycol, bal ? 63 - __clzll(bal) : lane);
        safe = bal ? lastcol : safe;
        __builtin_amdgcn_wave_barrier();
        mrow[gbase + (kp ? pos : kcnt + (sub - pos))] = kp ? mycol : safe;
        __builtin_amdgcn_wave_barrier();
        {
            int e = base + LPR + sub;
            e = (e < last) ? e : last;
            np = __builtin_nontemporal_load(pp + e);
        }
        const int32_t *mg = mrow + gbase;
#pragma unroll
        for (int k = 0; k < LPR; k += U) {
            if (!__any(k < kcnt)) break;
            // U independent row loads, unpredicated and back to back; in a ragged batch the places at or beyond kcnt re-read the
            // group's last kept row and are kept out of the sum by `ok` (a select, not a product: whatever that row holds)
            int32_t c[U];
            float x[U][VEC];
            if constexpr (U >= 4) {
#pragma unroll
                for (int u = 0; u < U; u += 4) {
                    const int4 m = *reinterpret_cast<const int4 *>(mg + k + u);
                    c[u] = m.x; c[u + 1] = m.y; c[u + 2] = m.z; c[u + 3] = m.w;
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) c[u] = mg[k + u];
            }
            if (fact) {
#pragma unroll
                for (int u = 0; u < U; ++u) vload<VEC>(x[u], row_at<OFF32>(B, lane_off, c[u], ldb));
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool ok = k + u < kcnt;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] += ok ? x[u][v] : 0.f;     // (acc is never -0.0: adding +0.0 keeps its bits)
                }
            }
        }
    }

    if (tact && fact) {
        if (t.dst >= 0) {
            vstore<VEC>(partial + (int64_t)t.dst * f + fcol, acc);
        } else {
            float *o = C + (int64_t)(~t.dst) * ldc + fcol;
            if (flags & PGCN_SPMM_ACCUMULATE) {
                float oc[VEC];
                vload<VEC>(oc, o);
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = oc[v] + acc[v];
            }
            vstore<VEC>(o, acc);
        }
    }
}

// kCountLanes lanes per task, no rows loaded.  A direct row is written (or added to) by its one task; the pieces of a cut row are
// added with integer atomics onto counts the entry point zeroed (exact in any order).
__global__ __launch_bounds__(kThreads) void dropedge_count_kernel(
    const int64_t *__restrict__ rowptr, const uint64_t *__restrict__ pairs, const int4 *__restrict__ tasks, int64_t ntasks,
    const int32_t *__restrict__ rowgid, const int32_t *__restrict__ slot_row, int32_t *__restrict__ count, uint32_t flags,
    uint64_t seed, const int64_t *__restrict__ step, uint32_t thr) {
    constexpr int G = 64 / kCountLanes;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int sub = lane % kCountLanes;
    const int64_t tid = ((int64_t)blockIdx.x * kWaves + wave) * G + lane / kCountLanes;
    const bool tact = tid < ntasks;
    const Task t = read_task(tasks, rowptr, tid, tact);
    const uint32_t gi = task_gid(t, tact, rowgid, slot_row);
    const uint64_t key = dropedge_key(seed, (uint64_t)step[0]);
    int n = 0;
    for (int e = sub; e < t.len; e += kCountLanes) {
        const uint64_t p = __builtin_nontemporal_load(pairs + t.kbeg + e);
        n += dropedge_keep(key, gi, (uint32_t)(p >> 32), thr) ? 1 : 0;
    }
#pragma unroll
    for (int off = kCountLanes / 2; off >= 1; off >>= 1) n += __shfl_xor(n, off, kCountLanes);
    if (tact && sub == 0) {
        if (t.dst >= 0) {
            atomicAdd(count + slot_row[t.dst], n);
        } else {
            int32_t *o = count + (int64_t)(~t.dst);
            *o = ((flags & PGCN_SPMM_ACCUMULATE) ? *o : 0) + n;
        }
    }
}

__global__ __launch_bounds__(kThreads) void dropedge_scales_kernel(const int32_t *__restrict__ count, int64_t n, float *__restrict__ scale) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t c = count[i];
    scale[i] = c > 0 ? (float)(1.0 / sqrt((double)c)) : 1.0f;     // double sqrt, double division, rounded once to fp32
}

// Y[i, .] = s[i] * X[i, .]: the layout of pgcn_rowband.h; grid y walks the columns kMaxF at a time (any f)
template <bool VEC>
__global__ __launch_bounds__(kThreads) void row_scale_kernel(const float *X, int64_t ldx, const float *__restrict__ s, int64_t nrows, int f,
                                                             int log2_tpr, float *Y, int64_t ldy) {
#pragma clang fp contract(off)
    const int coff = blockIdx.y * kMaxF;
    const int fl = (f - coff < kMaxF) ? f - coff : kMaxF;
    const auto [tpr, u, rg, ngroups, c0, r0, rend] = band_of(log2_tpr, kApplyRows, nrows);
    if (c0 >= fl) return;
    X += coff;
    Y += coff;
    for (int64_t r = r0 + rg; r < rend; r += kRowsInFlight * (int64_t)ngroups) {
        Quad q[kRowsInFlight];
        float sc[kRowsInFlight];
#pragma unroll
        for (int k = 0; k < kRowsInFlight; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr < rend) {
                q[k] = load_quad<VEC>(X + rr * ldx, c0, fl);
                sc[k] = s[rr];
            }
        }
#pragma unroll
        for (int k = 0; k < kRowsInFlight; ++k) {
            const int64_t rr = r + (int64_t)k * ngroups;
            if (rr >= rend) break;
            Quad y;
#pragma unroll
            for (int j = 0; j < 4; ++j) y.v[j] = sc[k] * q[k].v[j];
            store_quad<VEC>(Y + rr * ldy, c0, fl, y);
        }
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

struct Grid { int64_t blocks, nblocks; int ntiles; };

template <int LPR, int VEC>
Grid task_grid(int64_t ntasks, int32_t f, uint32_t flags, int32_t nslices, const int64_t *seg_host, SliceSeg &seg) {
    const int64_t per_block = (int64_t)kWaves * (64 / LPR);
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
int launch_sum(const int64_t *rowptr, const int32_t *pairs, const int32_t *rowgid, const int32_t *slot_row, const int32_t *tasks,
               int64_t ntasks, const int64_t *seg_host, int32_t nslices, const float *B, int64_t ldb, float *C, int64_t ldc, int32_t f,
               float *partial, uint64_t seed, const int64_t *step, uint32_t thr, uint32_t flags, hipStream_t s) {
    SliceSeg seg{};
    const Grid g = task_grid<LPR, VEC>(ntasks, f, flags, nslices, seg_host, seg);
    if (g.blocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_sum_csr_plan_f32: too many tasks for one launch");
    const uint64_t *p64 = reinterpret_cast<const uint64_t *>(pairs);
    const int4 *t4 = reinterpret_cast<const int4 *>(tasks);
    if (flags & PGCN_SPMM_OFFSETS32)
        hipLaunchKernelGGL((dropedge_sum_kernel<LPR, VEC, true>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s, rowptr, p64, t4,
                           ntasks, rowgid, slot_row, B, ldb, C, ldc, f, partial, g.blocks, flags, nslices, seg, seed, step, thr);
    else
        hipLaunchKernelGGL((dropedge_sum_kernel<LPR, VEC, false>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s, rowptr, p64, t4,
                           ntasks, rowgid, slot_row, B, ldb, C, ldc, f, partial, g.blocks, flags, nslices, seg, seed, step, thr);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

}  // namespace

#define PGCN_DROPEDGE_SHAPES(CASE)                                                         \
    CASE(1, 4) CASE(2, 4) CASE(4, 4) CASE(8, 4) CASE(16, 4) CASE(32, 4) CASE(64, 4)        \
    CASE(1, 1) CASE(2, 1) CASE(4, 1) CASE(8, 1) CASE(16, 1) CASE(32, 1) CASE(64, 1)

extern "C" int pgcn_dropedge_sum_csr_plan_f32(const int64_t *rowptr, const int32_t *pairs, const int32_t *row_gid, const int32_t *slot_row,
                                              const int32_t *tasks, int64_t ntasks, const int64_t *seg, int32_t nslices,
                                              const int32_t *fix, int64_t nfix, const float *B, int64_t ldb, float *C, int64_t ldc,
                                              int32_t f, float *partial_ws, int64_t partial_ws_elems, int64_t nslots, uint64_t seed,
                                              const int64_t *step, uint32_t thr, uint32_t flags, pgcn_stream_t stream) {
    if (ntasks < 0 || nfix < 0 || nslots < 0 || f < 1 || ldb < f || ldc < f || nslices < 1 || nslices > PGCN_MAX_SLICES ||
        (nslices > 1 && (!seg || !tasks)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_sum_csr_plan_f32: bad sizes");
    if (nslices > 1 && (seg[0] != 0 || seg[nslices] != ntasks))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_sum_csr_plan_f32: seg does not cover the task list");
    if (ntasks == 0) return PGCN_OK;
    if (!rowptr || !pairs || !row_gid || !B || !C || !step || (nfix > 0 && (!fix || !tasks)) || (nslots > 0 && (!partial_ws || !slot_row)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_sum_csr_plan_f32: null pointer");
    if (ntasks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_sum_csr_plan_f32: ntasks >= 2^31");
    if ((uintptr_t)pairs % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_sum_csr_plan_f32: pairs must be 8-byte aligned");
    if (partial_ws_elems < nslots * (int64_t)f)
        return pgcn_set_error(PGCN_ENOMEM, "pgcn_dropedge_sum_csr_plan_f32: partial work-space too small");
    const Shape sh = pick_shape(f, aligned16(B) && aligned16(C) && aligned16(partial_ws) && ldb % 4 == 0 && ldc % 4 == 0 && f % 4 == 0, flags);
    int rc = 1;   // (no shape taken yet)
#define PGCN_CASE(L, V)                                                                                                            \
    if (sh.lpr == L && sh.vec == V)                                                                                                \
        rc = launch_sum<L, V>(rowptr, pairs, row_gid, slot_row, tasks, ntasks, seg, nslices, B, ldb, C, ldc, f, partial_ws, seed, step, \
                              thr, flags, (hipStream_t)stream);
    PGCN_DROPEDGE_SHAPES(PGCN_CASE)
#undef PGCN_CASE
    if (rc == 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_sum_csr_plan_f32: no kernel shape");
    if (rc != PGCN_OK || nfix == 0) return rc;
    // the pieces of a cut row, added in slot order (the sum path's fix-up: the slots hold plain partial sums)
    return pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_ws, C, ldc, f, flags & PGCN_SPMM_ACCUMULATE, stream);
}

extern "C" int pgcn_dropedge_count_csr_plan_i32(const int64_t *rowptr, const int32_t *pairs, const int32_t *row_gid,
                                                const int32_t *slot_row, const int32_t *tasks, int64_t ntasks, int64_t nslots,
                                                int64_t nrows, int32_t *count, uint64_t seed, const int64_t *step, uint32_t thr,
                                                uint32_t flags, pgcn_stream_t stream) {
    if (ntasks < 0 || nslots < 0 || nrows < 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_count_csr_plan_i32: bad sizes");
    if (nrows == 0) return PGCN_OK;
    if (!count) return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_count_csr_plan_i32: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (!(flags & PGCN_SPMM_ACCUMULATE)) PGCN_HIP_CHECK(hipMemsetAsync(count, 0, (size_t)nrows * sizeof(int32_t), s));
    if (ntasks == 0) return PGCN_OK;
    if (!rowptr || !pairs || !row_gid || !step || (nslots > 0 && (!slot_row || !tasks)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_count_csr_plan_i32: null pointer");
    if (!tasks && ntasks != nrows) return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_count_csr_plan_i32: no task list, but ntasks != nrows");
    if ((uintptr_t)pairs % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_count_csr_plan_i32: pairs must be 8-byte aligned");
    const int64_t per_block = (int64_t)kWaves * (64 / kCountLanes);
    const int64_t blocks = (ntasks + per_block - 1) / per_block;
    if (blocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_count_csr_plan_i32: too many tasks for one launch");
    hipLaunchKernelGGL(dropedge_count_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, rowptr, reinterpret_cast<const uint64_t *>(pairs),
                       reinterpret_cast<const int4 *>(tasks), ntasks, row_gid, slot_row, count, flags, seed, step, thr);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_dropedge_scales_f32(const int32_t *count, int64_t n, float *scale, pgcn_stream_t stream) {
    if (n < 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_scales_f32: n < 0");
    if (n == 0) return PGCN_OK;
    if (!count || !scale) return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_scales_f32: null pointer");
    const int64_t blocks = (n + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_dropedge_scales_f32: too many rows for one launch");
    hipLaunchKernelGGL(dropedge_scales_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, count, n, scale);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_row_scale_f32(const float *X, int64_t ldx, const float *s, int64_t nrows, int32_t f, float *Y, int64_t ldy,
                                  pgcn_stream_t stream) {
    if (nrows < 0 || f < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_row_scale_f32: nrows < 0 or f < 1");
    if (ldx < f || ldy < f) return pgcn_set_error(PGCN_EINVAL, "pgcn_row_scale_f32: a leading dimension is below f");
    if (nrows == 0) return PGCN_OK;
    if (!X || !s || !Y) return pgcn_set_error(PGCN_EINVAL, "pgcn_row_scale_f32: null pointer");
    if (Y == X && ldy != ldx) return pgcn_set_error(PGCN_EINVAL, "pgcn_row_scale_f32: in place (Y == X) needs equal leading dimensions");
    const int64_t blocks = apply_blocks(nrows);
    const int ytiles = (f + kMaxF - 1) / kMaxF;
    if (blocks > 0x7fffffffLL || ytiles > 65535) return pgcn_set_error(PGCN_EINVAL, "pgcn_row_scale_f32: too large for one launch");
    const bool vec = f % 4 == 0 && rows16(ldx) && rows16(ldy) && aligned16(X) && aligned16(Y);
    const int log2_tpr = log2_threads_per_row(f < kMaxF ? f : kMaxF);
    hipLaunchKernelGGL(vec ? row_scale_kernel<true> : row_scale_kernel<false>, dim3((unsigned)blocks, ytiles), dim3(kThreads), 0,
                       (hipStream_t)stream, X, ldx, s, nrows, f, log2_tpr, Y, ldy);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}
