// pgcn_gat_tasks.h -- the task / lane scaffolding shared by the attention passes over head-major planes (pgcn_gatv2.hip, pgcn_gatdot.hip).
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

}  // namespace
#endif
