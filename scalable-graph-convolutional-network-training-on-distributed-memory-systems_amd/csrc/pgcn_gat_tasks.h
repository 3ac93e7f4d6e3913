// pgcn_gat_tasks.h -- what the attention passes over head-major planes (pgcn_gatv2.hip, pgcn_gatdot.hip) share: the task / lane
// scaffolding, the store of a task's output row, pass 1 of the row gradient (attn_dalpha_kernel) and the host-side plan checks.
//
// One wave owns a task of the plan of pgcn_spmm_plan_host (a row, an XCD slice of it or a chunk of a long row), a lane owns four features
// of the heads * d <= 256 wide row, d / 4 lanes form a head.  Everything here has internal linkage: each translation unit gets its own copy.
#ifndef PGCN_GAT_TASKS_H
#define PGCN_GAT_TASKS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgcn_device.h"
#include "pgcn_internal.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kBatch = 8;
constexpr int kMaxHeads = 8;

struct SliceSeg { int64_t v[PGCN_MAX_SLICES + 1]; };

struct Plan {                          // the task list of pgcn_spmm_plan_host on the structure (tasks == NULL: one task per row)
    const int64_t *rowptr;
    const int32_t *col;
    const int4 *tasks;
    int64_t ntasks;
    int64_t nrows;
    int32_t nslices;
    SliceSeg seg;
};

struct Task {
    int64_t kbeg, row;
    int32_t len, dst;
    bool act;
};

__device__ __forceinline__ Task pick_task(const Plan &pl) {
    const int wave = threadIdx.x >> 6;
    int64_t tid, nt = pl.ntasks;
    if (pl.nslices > 1) {              // workgroup b runs on XCD b % 8 and takes tasks of slice b % nslices (see pgcn_spmm.hip)
        const int slice = blockIdx.x % pl.nslices;
        tid = pl.seg.v[slice] + (int64_t)(blockIdx.x / pl.nslices) * kWaves + wave;
        nt = pl.seg.v[slice + 1];
    } else {
        tid = (int64_t)blockIdx.x * kWaves + wave;
    }
    Task t{0, 0, 0, -1, tid < nt};
    if (!t.act) return t;
    if (pl.tasks) {
        const int4 q = pl.tasks[tid];
        t.kbeg = (int64_t)(((uint64_t)(uint32_t)q.y << 32) | (uint32_t)q.x);
        t.len = q.z;
        t.dst = q.w;
        if (t.dst < 0) {
            t.row = ~t.dst;
        } else {                       // largest row with rowptr[row] <= kbeg (a split row is never empty)
            int64_t lo = 0, hi = pl.nrows - 1;
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (pl.rowptr[mid] <= t.kbeg) lo = mid; else hi = mid - 1;
            }
            t.row = lo;
        }
    } else {
        t.row = tid;
        t.kbeg = pl.rowptr[tid];
        t.len = (int32_t)(pl.rowptr[tid + 1] - t.kbeg);
        t.dst = ~(int32_t)tid;
    }
    return t;
}

struct Lane {                          // a lane's place in the heads * d wide row
    int fcol, fsafe, head, sub;
    bool fact;
};

__device__ __forceinline__ Lane pick_lane(int32_t F, int32_t d) {
    const int lane = threadIdx.x & 63;
    Lane l;
    l.fcol = lane * 4;
    l.fact = l.fcol < F;
    l.fsafe = l.fact ? l.fcol : 0;     // (lanes beyond the F features gather column 0 and are never stored)
    l.head = l.fact ? l.fcol / d : 0;
    l.sub = lane & ((d >> 2) - 1);
    return l;
}

// the output row of a task: straight into C (its row's only task) or into its slot
__device__ __forceinline__ void put_row(const Task &t, const Lane &l, float (&acc)[4], float *__restrict__ C, int64_t ldc,
                                        float *__restrict__ partial, int32_t F, uint32_t flags) {
    if (!t.act || !l.fact) return;
    if (t.dst >= 0) {
        vstore<4>(partial + (int64_t)t.dst * F + l.fcol, acc);
    } else {
        float *cp = C + t.row * ldc + l.fcol;
        if (flags & PGCN_SPMM_ACCUMULATE) {
            float old[4];
            vload<4>(old, cp);
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[v] += old[v];
        }
        vstore<4>(cp, acc);
    }
}

// ---- pass 1 of the row gradient, over the forward structure: q_ij = <dOut_i, Zg_j - out_i> into the de planes, T_i = sum_j alpha_ij q_ij
// (Zg: the operand the forward pass aggregated -- Zs of a GATv2 layer, Zv of a dot-product layer).
//
// The row pass of both layers is TWO passes over the forward structure.  Mathematically sum_j de_ij = 0 for every row and head, and the
// row gradient (dZt and da of GATv2, dZq of the dot product) multiplies de by quantities of one sign and size along a row -- a
// LReLU(x_ij), or key rows that share a large common component: an error that all entries of a row SHARE -- the rounding of t_i =
// <dOut_i, out_i>, or of out_i -- does not cancel but comes back times sum_j alpha_ij LReLU(x_ij).  Where a row's softmax is nearly
// one-hot (scores of magnitude ~150) that shared error is the result: measured on such rows, da was 3.4e-3 from float64 with t =
// <dOut_i, out_i> from a separate dot and 2.3e-3 with de = alpha <dOut_i, Zs_j - out_i>, where the float32 statement of the definition
// is at 1.1e-3 (tests/test_gatv2_gpu.py).  So this pass writes q_ij into the de planes and T_i (slots and fix-up for cut rows), and
// pass 2 (gatv2_grad_rows_kernel, gatdot_grad_rows_kernel) forms de_ij = alpha_ij (q_ij - T_i) from THE SAME q: the rows of de then
// sum to zero to rounding, as in torch's own softmax backward.  One more gather of Zg (it is the pass's second touch of the same
// rows) buys that.
__global__ __launch_bounds__(kThreads) void attn_dalpha_kernel(Plan pl, const float *__restrict__ Zg, int64_t ldg,
                                                               const float *__restrict__ alpha, int64_t stride_a,
                                                               const float *__restrict__ dOut, int64_t ldo, const float *__restrict__ out,
                                                               int64_t ldout, int32_t heads, int32_t d, int32_t F, float *__restrict__ de,
                                                               int64_t stride_de, float *__restrict__ T, float *__restrict__ partial) {
    const Task t = pick_task(pl);
    if (!t.act) return;                        // (wave-uniform; no workgroup barrier below)
    const int lane = threadIdx.x & 63;
    const Lane l = pick_lane(F, d);
    const int hl = d >> 2;
    float g0[4] = {0.f, 0.f, 0.f, 0.f}, o4[4] = {0.f, 0.f, 0.f, 0.f};
    if (l.fact) {
        vload<4>(g0, dOut + t.row * ldo + l.fcol);
        vload<4>(o4, out + t.row * ldout + l.fcol);
    }
    const float *ak = alpha + (int64_t)l.head * stride_a + t.kbeg;
    float *dk = de + (int64_t)l.head * stride_de + t.kbeg;
    float tacc = 0.f;                          // (the same on every lane of a head)
    const int last = t.len > 0 ? t.len - 1 : 0;
    for (int base = 0; base < t.len; base += 64) {
        const int el = base + lane < last ? base + lane : last;
        const int32_t cl = pl.col[t.kbeg + el];
        const int cnt = min(64, t.len - base);
        for (int e0 = 0; e0 < cnt; e0 += kBatch) {
            float x[kBatch][4], al[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int e = e0 + u < cnt ? e0 + u : cnt - 1;
                const int32_t c = __shfl(cl, e, 64);
                vload<4>(x[u], Zg + (int64_t)c * ldg + l.fsafe);
                al[u] = ak[base + e];
            }
            float p[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u)
                p[u] = (g0[0] * (x[u][0] - o4[0]) + g0[1] * (x[u][1] - o4[1])) + (g0[2] * (x[u][2] - o4[2]) + g0[3] * (x[u][3] - o4[3]));
            for (int o = hl >> 1; o > 0; o >>= 1) {
#pragma unroll
                for (int u = 0; u < kBatch; ++u) p[u] += __shfl_xor(p[u], o, 64);
            }
            float pm = p[0];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                tacc += e0 + u < cnt ? al[u] * p[u] : 0.f;
                pm = l.sub == u ? p[u] : pm;
            }
            const int e = e0 + l.sub;
            if (l.fact && l.sub < kBatch && e < cnt) dk[base + e] = pm;
        }
    }
    if (l.fact && l.sub == 0) (t.dst >= 0 ? partial + (int64_t)t.dst * heads : T + t.row * heads)[l.head] = tacc;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
int64_t plan_grid(bool has_tasks, int64_t nrows, int64_t ntasks, const int64_t *seg, int32_t nslices) {
    if (nslices > 1) {
        int64_t longest = 0;
        for (int i = 0; i < nslices; ++i) longest = seg[i + 1] - seg[i] > longest ? seg[i + 1] - seg[i] : longest;
        return ((longest + kWaves - 1) / kWaves) * nslices;
    }
    const int64_t nt = has_tasks ? ntasks : nrows;
    return (nt + kWaves - 1) / kWaves;
}

// sizes and shape limits shared by every entry point that walks a plan; PGCN_OK, or the code to return
int check_plan(const char *who, int32_t heads, int32_t d, int64_t nrows, const int32_t *tasks, int64_t ntasks, const int64_t *seg,
               int32_t nslices, Plan *pl, int64_t *grid) {
    if (heads <= 0 || d <= 0 || nrows < 0 || ntasks < 0 || nslices < 1 || nslices > PGCN_MAX_SLICES || (nslices > 1 && (!seg || !tasks)))
        return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes");
    const int hl = d / 4;
    if (heads > kMaxHeads || (int64_t)heads * d > 256 || d % 4 || hl < kBatch || (hl & (hl - 1)))
        return pgcn_set_error2(PGCN_EUNSUPPORTED, who, "needs heads <= 8, d = 32, 64, 128 or 256 and heads * d <= 256");
    if (nslices > 1 && (seg[0] != 0 || seg[nslices] != ntasks)) return pgcn_set_error2(PGCN_EINVAL, who, "seg does not cover the task list");
    pl->tasks = reinterpret_cast<const int4 *>(tasks);
    pl->ntasks = tasks ? ntasks : nrows;
    pl->nrows = nrows;
    pl->nslices = nslices;
    for (int i = 0; i <= PGCN_MAX_SLICES; ++i) pl->seg.v[i] = (nslices > 1 && i <= nslices) ? seg[i] : 0;
    *grid = plan_grid(tasks != nullptr, nrows, ntasks, seg, nslices);
    if (*grid > 0x7fffffffLL) return pgcn_set_error2(PGCN_EINVAL, who, "too many tasks for one launch");
    return PGCN_OK;
}

bool bad_rows(const float *p, int64_t ld) { return ld % 4 || (uintptr_t)p % 16; }

}  // namespace
#endif
