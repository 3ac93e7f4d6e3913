// pgcn_gat_attndrop.hip -- the two gather passes of a GAT layer under ATTENTION DROPOUT (gfx950), fp32: the masked twins of the FWD
// and GRAD instantiations of spmm_heads_kernel (pgcn_spmm_heads.hip).  include/pgcn_hip.h has the contract, pgcn_attndrop.h the keep
// function, DESIGN.md section 4 the arithmetic.
//
//   alpha'_ijk = keep(i, j, k) ? alpha_ijk * scale : 0        alpha: the edge softmax over the WHOLE row (dropout comes after it)
//   c_ijk = alpha_ijk LeakyReLU'(s1_ik + s2_jk),   c'_ijk = keep ? c_ijk * scale : 0
//   forward   out_i = sum_j alpha'_ij Z_j,  V_i = sum_j c'_ij Z_j,  C_i = sum_j c_ij  (UNMASKED: a dropped entry still pulls on the
//             scores through the normalisation)                                                    pgcn_gat_attndrop_forward2_f32
//   backward  (transposed structure)  dZ_j = sum_i alpha'_ij dOut_i,  ds2_j = sum_i (c'_ij <dOut_i, Z_j> - c_ij t_i),
//             t_i = <dOut_i, out_i> of the MASKED out                                              pgcn_gat_attndrop_grad_f32
//
// Mapping to the machine: that of spmm_heads_kernel.  One wave owns a task of the plan (a row, an XCD slice or a chunk of a long row),
// a lane owns four features of the K*d <= 256 wide row, 64 entries are prepared lane-parallel and parked in the wave's LDS, the rows
// are gathered in unpredicated batches of 8, cut rows go through slots and pgcn_spmm_fixup_f32 in slot order: fixed summation order,
// no atomics.  The mask lives in the lane-parallel stage: the lane that recomputes the weights of an entry also fetches the two
// global ids (the task's own row: one value per wave; the entry's column: one 4-byte gather) and evaluates the K keep bits -- one
// hash evaluation per entry and WAVE (2 + K fmix32 forward, 1 + K backward, where the neighbour's share belongs to the task), not
// one per lane and entry.  A dropped entry's parked weight is an exact 0 from a select; its row is gathered like any other (the
// gathers stay unpredicated, and an entry is dropped per head: its row is needed unless all K heads drop it).
//   forward:  parked words per entry 2 K + 1 (col, alpha', c'); C is summed from the unmasked c in registers before parking.
//   backward: parked words per entry 3 K + 1 (col, alpha', c', c t): de = c' dp - c t needs no fourth group.
// The step is read from DEVICE memory: a captured training step draws a new mask at every replay.  Mode 0 (LeakyReLU + softmax over
// the neighbours) only; no per-entry gradient output.  Plain vector loads and stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgcn_device.h"
#include "pgcn_internal.h"

#define PG_DROPOUT_FN __host__ __device__ __forceinline__
#include "../gemm/pgcn_dropout.h"
#include "pgcn_attndrop.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kBatch = 8;
constexpr int kMaxHeads = 8;

using f32x2 = __attribute__((ext_vector_type(2))) float;

// x of another lane of the same 16-lane row through the DPP network (CTRL: 0x120 + n = row_ror:n, 0x00-0xFF = quad_perm)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
// lane ^ 4 inside a 16-lane row: row_shl:4 serves the lanes of banks 0 and 2, row_shr:4 those of banks 1 and 3
__device__ __forceinline__ float dpp_xor4(float x) {
    const int v = __float_as_int(x);
    int r = __builtin_amdgcn_update_dpp(0, v, 0x104, 0xF, 0x5, false);
    r = __builtin_amdgcn_update_dpp(r, v, 0x114, 0xF, 0xA, false);
    return __int_as_float(r);
}

struct SliceSeg { int64_t v[PGCN_MAX_SLICES + 1]; };

struct Stats {                   // the softmax's statistics: of the task's row (forward) or of the entry's column (backward)
    const float4 *rowstat;       // [. x KH] (s1, m, 1/D, 0)
    const float *s2;             // forward: [ncols x lds2] of the entry's column; backward: [nrows x lds2] of the task's row
    int64_t lds2;
    int64_t nrows;
    float slope;
};

struct Mask {                    // pgcn_attndrop.h
    const int32_t *row_gid;      // [nrows] global ids of the structure's rows (forward: gi, backward: gj)
    const int32_t *col_gid;      // [ncols] ... of its columns             (forward: gj, backward: gi)
    uint64_t seed;
    const int64_t *step;         // one int64 in device memory
    uint64_t layer;
    uint32_t thr;
    float scale;
};

struct EdgeGrad {                // backward: what the edge gradient needs on top of Stats
    const float *Z;              // [nrows x ldz] Z_j of the task's row
    int64_t ldz;
    const float *t;              // [ncols x KH] t_i = <dOut_i, out_i>
    int32_t pw;                  // width of a partial / output row: F + heads rounded up to 4
};

struct Forward2 {                // forward: the second output
    float *C2;                   // [nrows x ldc2]: V in columns [0, F), C in [F, F + KH), zeros up to pw2
    int64_t ldc2;
    float *partial2;             // slot rows of pw2 floats (behind the F-wide slot rows of the first output)
    int32_t pw2;                 // F + heads rounded up to 4
};

template <int KH, bool GRAD>
__global__ __launch_bounds__(kThreads, (GRAD || KH > 4) ? 4 : 5) void attndrop_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int4 *__restrict__ tasks, int64_t ntasks,
    const float *__restrict__ B, int64_t ldb, float *__restrict__ C, int64_t ldc, int32_t F, int32_t d, float *__restrict__ partial,
    uint32_t flags, int32_t nslices, SliceSeg seg, Stats rc, EdgeGrad eg, Forward2 f2, Mask mk) {
    constexpr bool FWD = !GRAD;
    // parked words per entry: col, alpha'[KH], c'[KH] (GRAD: also (c t)[KH])
    constexpr int PS = GRAD ? 3 * KH + 1 : 2 * KH + 1;
    __shared__ float park[kWaves][64 * PS];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    int64_t tid;
    if (nslices > 1) {   // workgroup b runs on XCD b % 8 and takes tasks of slice b % nslices (see pgcn_spmm.hip)
        const int slice = blockIdx.x % nslices;
        tid = seg.v[slice] + (int64_t)(blockIdx.x / nslices) * kWaves + wave;
        ntasks = seg.v[slice + 1];
    } else {
        tid = (int64_t)blockIdx.x * kWaves + wave;
    }
    const bool tact = tid < ntasks;
    int32_t len = 0, dst = -1;
    int64_t kbeg = 0;
    if (tact) {
        if (tasks) {
            const int4 t = tasks[tid];
            kbeg = (int64_t)(((uint64_t)(uint32_t)t.y << 32) | (uint32_t)t.x);
            len = t.z;
            dst = t.w;
        } else {
            kbeg = rowptr[tid];
            len = (int32_t)(rowptr[tid + 1] - kbeg);
            dst = ~(int32_t)tid;
        }
    }
    const int fcol = lane * 4;
    const bool fact = fcol < F;
    const int fsafe = fact ? fcol : 0;
    const int head = fact ? fcol / d : 0;
    f32x2 accl = {0.f, 0.f}, acch = {0.f, 0.f};        // this lane's four features of the output row
    f32x2 vl = {0.f, 0.f}, vh = {0.f, 0.f};            // forward: ... and of V
    float csum[KH];                                    // forward: this lane's share of C_i (unmasked)
#pragma unroll
    for (int k = 0; k < KH; ++k) csum[k] = 0.f;
    float *mine = park[wave];
    const int last = len > 0 ? len - 1 : 0;
    float a2[KH];                          // backward: s2 of this task's row
#pragma unroll
    for (int k = 0; k < KH; ++k) a2[k] = 0.f;
    int64_t row = 0;
    uint32_t rgid = 0;                     // global id of the task's row
    if (len > 0) {
        if (dst < 0) {
            row = ~dst;
        } else {                         // largest row with rowptr[row] <= kbeg (a split row is never empty)
            int64_t lo = 0, hi = rc.nrows - 1;
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (rowptr[mid] <= kbeg) lo = mid; else hi = mid - 1;
            }
            row = lo;
        }
        rgid = (uint32_t)mk.row_gid[row];
        if constexpr (GRAD) {
#pragma unroll
            for (int k = 0; k < KH; ++k) a2[k] = rc.s2[row * rc.lds2 + k];
        }
    }
    const uint64_t key = attndrop_key(mk.seed, (uint64_t)mk.step[0], mk.layer);
    // what the task's row contributes to every entry's hash: backward, the row is the NEIGHBOUR gj (its share is one fmix32, once)
    const uint32_t rshare = GRAD ? attndrop_col(key, rgid) : rgid;
    // backward: this lane's four features of Z_j, the lanes of a head, and which entry of a batch the lane finishes
    f32x2 zl = {0.f, 0.f}, zh = {0.f, 0.f};
    const int hl = d >> 2;                 // lanes per head (the host admits powers of two >= kBatch only)
    const int u_mine = hl == 16 ? (lane & 15) >> 1 : lane & (hl - 1);
    const bool writer = hl == 16 ? !(lane & 1) : u_mine < kBatch;
    float acc2 = 0.f;
    if constexpr (GRAD) {
        if (len > 0 && fact) {
            float zr[4];
            vload<4>(zr, eg.Z + row * eg.ldz + fcol);
            zl = f32x2{zr[0], zr[1]};
            zh = f32x2{zr[2], zr[3]};
        }
    }
    // the weights of the entry with column c: w = alpha', ga = c', gx = c (forward: unmasked, for C_i) or c t (backward)
    auto weights = [&](int32_t c, float (&w)[KH], float (&ga)[KH], float (&gx)[KH]) {
        const uint32_t cg = (uint32_t)mk.col_gid[c];
        const uint32_t b = GRAD ? attndrop_entry(key, rshare, cg) : attndrop_entry(key, attndrop_col(key, cg), rshare);
        float4 q[KH];
        float sv[KH], tv[KH];
        if constexpr (FWD) {               // (statistics of the task's row: one line, the same for all lanes, re-read per 64 entries)
#pragma unroll
            for (int k = 0; k < KH; ++k) q[k] = rc.rowstat[row * KH + k];
#pragma unroll
            for (int k = 0; k < KH; ++k) sv[k] = rc.s2[(int64_t)c * rc.lds2 + k];
        } else {
#pragma unroll
            for (int k = 0; k < KH; ++k) q[k] = rc.rowstat[(int64_t)c * KH + k];
#pragma unroll
            for (int k = 0; k < KH; ++k) tv[k] = eg.t[(int64_t)c * KH + k];
        }
#pragma unroll
        for (int k = 0; k < KH; ++k) {
            const float raw = q[k].x + (FWD ? sv[k] : a2[k]);
            const float r = raw > 0.f ? raw : raw * rc.slope;
            const float al = (expf(r - q[k].y) - q[k].w) * q[k].z;
            const float cc = al * (raw > 0.f ? 1.f : rc.slope);
            const bool keep = attndrop_head(b, (uint32_t)k) >= mk.thr;
            w[k] = keep ? al * mk.scale : 0.f;
            ga[k] = keep ? cc * mk.scale : 0.f;
            gx[k] = FWD ? cc : cc * tv[k];
        }
    };
    // prefetch of the first 64 tuples: unconditional, index clamped into the task
    int32_t nc = 0;
    float na[KH], nga[KH], ngx[KH];
#pragma unroll
    for (int k = 0; k < KH; ++k) na[k] = nga[k] = ngx[k] = 0.f;
    if (len > 0) {
        const int e = lane < last ? lane : last;
        nc = __builtin_nontemporal_load(col + kbeg + e);
        weights(nc, na, nga, ngx);
        if constexpr (FWD) {
#pragma unroll
            for (int k = 0; k < KH; ++k) csum[k] += lane < len ? ngx[k] : 0.f;
        }
    }
    for (int base = 0; base < len; base += 64) {   // wave-uniform: one task per wave
        __builtin_amdgcn_wave_barrier();
        mine[lane * PS] = __int_as_float(nc);
#pragma unroll
        for (int k = 0; k < KH; ++k) {
            mine[lane * PS + 1 + k] = na[k];
            mine[lane * PS + 1 + KH + k] = nga[k];
        }
        if constexpr (GRAD) {
#pragma unroll
            for (int k = 0; k < KH; ++k) mine[lane * PS + 1 + 2 * KH + k] = ngx[k];
        }
        __builtin_amdgcn_wave_barrier();
        if (base + 64 < len) {
            int e = base + 64 + lane;
            e = e < last ? e : last;
            nc = __builtin_nontemporal_load(col + kbeg + e);
            weights(nc, na, nga, ngx);
            if constexpr (FWD) {
#pragma unroll
                for (int k = 0; k < KH; ++k) csum[k] += base + 64 + lane < len ? ngx[k] : 0.f;
            }
        }
        const int cnt = min(64, len - base);
        // backward: the dot products of a batch are FINISHED (16-lane reduction, de, row sum) one batch later, after the next batch's
        // gathers have gone out: the reduction's chain of cross-lane round trips runs under their latency
        float dq[kBatch];
        int pe0 = -1;                          // first entry of the batch whose dot products are pending
        auto finish = [&](int e0p) {
            float dm;
            if (hl == 16) {
                // 8 entries x 16 lanes: a transposing reduction on the DPP network.  Lane l of the head ends with entry l >> 1.
                const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2;
                float r1[4], r2[2];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    r1[u] = (b3 ? dq[u + 4] : dq[u]) + dpp_f<0x128>(b3 ? dq[u] : dq[u + 4]);          // row_ror:8 = lane ^ 8
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    r2[u] = (b2 ? r1[u + 2] : r1[u]) + dpp_xor4(b2 ? r1[u] : r1[u + 2]);
                const float r3 = (b1 ? r2[1] : r2[0]) + dpp_f<0x4E>(b1 ? r2[0] : r2[1]);               // quad_perm [2,3,0,1]
                dm = r3 + dpp_f<0xB1>(r3);                                                            // quad_perm [1,0,3,2]
            } else {
                for (int o = hl >> 1; o > 0; o >>= 1) {
#pragma unroll
                    for (int u = 0; u < kBatch; ++u) dq[u] += __shfl_xor(dq[u], o, 64);
                }
                dm = dq[0];
#pragma unroll
                for (int u = 1; u < kBatch; ++u) dm = u_mine == u ? dq[u] : dm;
            }
            const int e = e0p + u_mine;        // the entry of the batch this lane finishes
            if (fact && writer && e < cnt)     // de = c' dp - c t (not stored: its row sum is ds2)
                acc2 += mine[e * PS + 1 + KH + head] * dm - mine[e * PS + 1 + 2 * KH + head];
        };
        for (int e0 = 0; e0 < cnt; e0 += kBatch) {
            int32_t c[kBatch];
            float w[kBatch], w2[kBatch];
            float x[kBatch][4];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int e = e0 + u < cnt ? e0 + u : cnt - 1;       // ragged tail: the task's last referenced row
                c[u] = __float_as_int(mine[e * PS]);
                w[u] = mine[e * PS + 1 + head];
                w2[u] = FWD ? mine[e * PS + 1 + KH + head] : 0.f;
            }
            // (lanes beyond the F features gather column 0 and are never stored: no branch around the gathers)
#pragma unroll
            for (int u = 0; u < kBatch; ++u) vload<4>(x[u], B + (int64_t)c[u] * ldb + fsafe);
            if constexpr (GRAD) {
                __builtin_amdgcn_sched_barrier(0);     // the gathers are out; nothing below may be moved above them,
                if (pe0 >= 0) finish(pe0);             // and no use of a gathered row above the pending reduction
#pragma unroll
                for (int u = 0; u < kBatch; ++u) dq[u] = 0.f;
                pe0 = e0;
                __builtin_amdgcn_sched_barrier(0);
            }
            if (e0 + kBatch <= cnt) {                  // full batches: packed FMAs, no selects
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    const f32x2 ww = {w[u], w[u]};
                    const f32x2 xl = {x[u][0], x[u][1]}, xh = {x[u][2], x[u][3]};
                    accl = __builtin_elementwise_fma(ww, xl, accl);
                    acch = __builtin_elementwise_fma(ww, xh, acch);
                    if constexpr (FWD) {
                        const f32x2 w22 = {w2[u], w2[u]};
                        vl = __builtin_elementwise_fma(w22, xl, vl);
                        vh = __builtin_elementwise_fma(w22, xh, vh);
                    }
                    if constexpr (GRAD) {
                        const f32x2 pr = __builtin_elementwise_fma(xh, zh, xl * zl);
                        dq[u] = pr.x + pr.y;
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    const bool in = e0 + u < cnt;
                    const float wk = in ? w[u] : 0.f;
                    const f32x2 ww = {wk, wk};
                    const f32x2 xl = {in ? x[u][0] : 0.f, in ? x[u][1] : 0.f}, xh = {in ? x[u][2] : 0.f, in ? x[u][3] : 0.f};
                    accl = __builtin_elementwise_fma(ww, xl, accl);
                    acch = __builtin_elementwise_fma(ww, xh, acch);
                    if constexpr (FWD) {
                        const float w2k = in ? w2[u] : 0.f;
                        const f32x2 w22 = {w2k, w2k};
                        vl = __builtin_elementwise_fma(w22, xl, vl);
                        vh = __builtin_elementwise_fma(w22, xh, vh);
                    }
                    if constexpr (GRAD) {
                        const f32x2 pr = __builtin_elementwise_fma(xh, zh, xl * zl);
                        dq[u] = pr.x + pr.y;
                    }
                }
            }
        }
        if constexpr (GRAD) {
            if (pe0 >= 0) finish(pe0);         // (before the next 64 entries overwrite the parked words)
        }
    }
    const int64_t pw = GRAD ? (int64_t)eg.pw : (int64_t)F;     // width of a partial row
    if constexpr (GRAD) {
        // ds2 of the row = sum of this task's de per head: lane L < pw - F writes column F + L (pad columns: zero)
        for (int o = hl >> 1; o > 0; o >>= 1) acc2 += __shfl_xor(acc2, o, 64);
        const int src = (lane < KH ? lane : KH - 1) * hl;
        const float v = __shfl(acc2, src, 64);
        if (tact && lane < eg.pw - F) {
            float out = lane < KH ? v : 0.f;
            if (dst >= 0) {
                partial[(int64_t)dst * pw + F + lane] = out;
            } else {
                float *cp = C + (int64_t)(~dst) * ldc + F + lane;
                if (flags & PGCN_SPMM_ACCUMULATE) out += *cp;
                *cp = out;
            }
        }
    }
    if constexpr (FWD) {
        // V_i beside the output row; C_i = the wave's sum of c_ij per head: lane L < pw2 - F writes column F + L
        float mysum = 0.f;
#pragma unroll
        for (int k = 0; k < KH; ++k) {
            float v = csum[k];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            mysum = lane == k ? v : mysum;
        }
        if (tact) {
            float *o2 = dst >= 0 ? f2.partial2 + (int64_t)dst * f2.pw2 : f2.C2 + (int64_t)(~dst) * f2.ldc2;
            const bool add = dst < 0 && (flags & PGCN_SPMM_ACCUMULATE);
            if (fact) {
                float v4[4] = {vl.x, vl.y, vh.x, vh.y};
                if (add) {
                    float old[4];
                    vload<4>(old, o2 + fcol);
#pragma unroll
                    for (int v = 0; v < 4; ++v) v4[v] += old[v];
                }
                vstore<4>(o2 + fcol, v4);
            }
            if (lane < f2.pw2 - F) {
                float out = lane < KH ? mysum : 0.f;
                if (add) out += o2[F + lane];
                o2[F + lane] = out;
            }
        }
    }
    float acc[4] = {accl.x, accl.y, acch.x, acch.y};
    if (tact && fact) {
        if (dst >= 0) {
            vstore<4>(partial + (int64_t)dst * pw + fcol, acc);
        } else {
            float *cp = C + (int64_t)(~dst) * ldc + fcol;
            if (flags & PGCN_SPMM_ACCUMULATE) {
                float old[4];
                vload<4>(old, cp);
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[v] += old[v];
            }
            vstore<4>(cp, acc);
        }
    }
}

int launch_attndrop(const char *who, const int64_t *rowptr, const int32_t *col, const Stats &rc, const EdgeGrad *eg, const Forward2 *f2,
                    const Mask &mk, int32_t layer, int32_t heads, int32_t d, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                    const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const float *B, int64_t ldb, float *C,
                    int64_t ldc, float *partial_ws, int64_t partial_ws_elems, int64_t nslots, uint32_t flags, pgcn_stream_t stream) {
    const int64_t F = (int64_t)heads * d;
    if (heads <= 0 || d <= 0 || nrows < 0 || ntasks < 0 || nfix < 0 || nslices < 1 || nslices > PGCN_MAX_SLICES || ldb < F || ldc < F ||
        (nslices > 1 && (!seg || !tasks)) || layer < 0 || (uint64_t)layer >= (1ull << 20))
        return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes");
    const int hl = d / 4;
    if (heads > kMaxHeads || F > 256 || d % 4 || hl < kBatch || (hl & (hl - 1)) || ldb % 4 || ldc % 4 || (uintptr_t)B % 16 ||
        (uintptr_t)C % 16 || (uintptr_t)partial_ws % 16)
        return pgcn_set_error2(PGCN_EUNSUPPORTED, who, "needs heads <= 8, d = 32, 64, 128 or 256, heads * d <= 256 and 16-byte aligned operands");
    const int64_t nt = tasks ? ntasks : nrows;
    if (nt == 0) return PGCN_OK;
    if (!rowptr || !col || !B || !C || (nfix > 0 && !fix) || (nslots > 0 && !partial_ws))
        return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    if (!rc.rowstat || !rc.s2 || rc.lds2 < heads || (uintptr_t)rc.rowstat % 16)
        return pgcn_set_error2(PGCN_EINVAL, who, "bad row statistics / s2");
    if (!mk.row_gid || !mk.col_gid || !mk.step)
        return pgcn_set_error2(PGCN_EINVAL, who, "the mask needs row_gid, col_gid and step");
    const int64_t pwx = F + (heads + 3) / 4 * 4;      // F + heads rounded up to 4
    int64_t pw = F, pw_all = F;                        // width of a first-output slot row; floats of work-space per slot
    Forward2 h0{};
    EdgeGrad g0{};
    if (eg) {
        if (!eg->Z || !eg->t || eg->ldz < F || eg->ldz % 4 || (uintptr_t)eg->Z % 16) return pgcn_set_error2(PGCN_EINVAL, who, "bad Z / t");
        if (ldc < pwx) return pgcn_set_error2(PGCN_EINVAL, who, "C must hold heads * d + heads (rounded up to 4) columns");
        pw = pw_all = pwx;
        g0 = *eg;
    } else {
        if (!f2->C2 || f2->ldc2 < pwx || f2->ldc2 % 4 || (uintptr_t)f2->C2 % 16)
            return pgcn_set_error2(PGCN_EINVAL, who, "bad second output (heads * d + heads columns, rounded up to 4)");
        pw_all = F + pwx;
        h0 = *f2;
        h0.partial2 = partial_ws ? partial_ws + nslots * F : nullptr;
    }
    if (nslots < 0 || partial_ws_elems < nslots * pw_all) return pgcn_set_error2(PGCN_ENOMEM, who, "partial work-space too small");
    SliceSeg sg{};
    int64_t grid;
    if (nslices > 1) {
        if (seg[0] != 0 || seg[nslices] != ntasks) return pgcn_set_error2(PGCN_EINVAL, who, "seg does not cover the task list");
        int64_t longest = 0;
        for (int i = 0; i <= nslices; ++i) sg.v[i] = seg[i];
        for (int i = 0; i < nslices; ++i) longest = sg.v[i + 1] - sg.v[i] > longest ? sg.v[i + 1] - sg.v[i] : longest;
        grid = ((longest + kWaves - 1) / kWaves) * nslices;
    } else {
        grid = (nt + kWaves - 1) / kWaves;
    }
    if (grid > 0x7fffffffLL) return pgcn_set_error2(PGCN_EINVAL, who, "too many tasks for one launch");
    if (grid == 0) return PGCN_OK;
    hipStream_t s = (hipStream_t)stream;
    const int4 *t4 = reinterpret_cast<const int4 *>(tasks);
#define PGCN_ATTNDROP_LAUNCH(KH, GR)                                                                                          \
    hipLaunchKernelGGL((attndrop_kernel<KH, GR>), dim3((unsigned)grid), dim3(kThreads), 0, s, rowptr, col, t4, nt, B, ldb, C, ldc, \
                       (int32_t)F, d, partial_ws, flags, nslices, sg, rc, g0, h0, mk)
#define PGCN_ATTNDROP(KH)                                 \
    case KH:                                              \
        if (eg) PGCN_ATTNDROP_LAUNCH(KH, true);           \
        else PGCN_ATTNDROP_LAUNCH(KH, false);             \
        break;
    switch (heads) {
        PGCN_ATTNDROP(1) PGCN_ATTNDROP(2) PGCN_ATTNDROP(3) PGCN_ATTNDROP(4) PGCN_ATTNDROP(5) PGCN_ATTNDROP(6) PGCN_ATTNDROP(7) PGCN_ATTNDROP(8)
    }
#undef PGCN_ATTNDROP
#undef PGCN_ATTNDROP_LAUNCH
    PGCN_HIP_CHECK(hipGetLastError());
    if (nfix > 0) {    // (backward: the ds2 columns of a split row are combined with its features, one list, one launch)
        const int rcf = pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_ws, C, ldc, (int32_t)pw, flags & PGCN_SPMM_ACCUMULATE, stream);
        if (rcf != PGCN_OK || eg) return rcf;
        return pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, h0.partial2, h0.C2, h0.ldc2, h0.pw2, flags & PGCN_SPMM_ACCUMULATE, stream);
    }
    return PGCN_OK;
}

}  // namespace

extern "C" int pgcn_gat_attndrop_forward2_f32(const int64_t *rowptr, const int32_t *col, const float *rowstat, const float *s2,
                                              int64_t lds2, float slope, int32_t heads, int32_t d, int64_t nrows,
                                              const int32_t *tasks, int64_t ntasks, const int64_t *seg, int32_t nslices,
                                              const int32_t *fix, int64_t nfix, const float *B, int64_t ldb, float *C, int64_t ldc,
                                              float *C2, int64_t ldc2, float *partial_ws, int64_t partial_ws_elems, int64_t nslots,
                                              uint32_t flags, const int32_t *row_gid, const int32_t *col_gid, uint64_t seed,
                                              const int64_t *step, int32_t layer, uint32_t thr, pgcn_stream_t stream) {
    const Stats rc{reinterpret_cast<const float4 *>(rowstat), s2, lds2, nrows, slope};
    const Forward2 f2{C2, ldc2, nullptr, heads * d + (heads + 3) / 4 * 4};
    const Mask mk{row_gid, col_gid, seed, step, (uint64_t)(layer < 0 ? 0 : layer), thr, dropout_scale(thr)};
    return launch_attndrop("pgcn_gat_attndrop_forward2_f32", rowptr, col, rc, nullptr, &f2, mk, layer, heads, d, nrows, tasks, ntasks, seg,
                           nslices, fix, nfix, B, ldb, C, ldc, partial_ws, partial_ws_elems, nslots, flags, stream);
}

extern "C" int pgcn_gat_attndrop_grad_f32(const int64_t *rowptr, const int32_t *col, const float *rowstat, const float *s2,
                                          int64_t lds2, float slope, int32_t heads, int32_t d, int64_t nrows, const int32_t *tasks,
                                          int64_t ntasks, const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix,
                                          const float *B, int64_t ldb, const float *Z, int64_t ldz, const float *t, float *C,
                                          int64_t ldc, float *partial_ws, int64_t partial_ws_elems, int64_t nslots, uint32_t flags,
                                          const int32_t *row_gid, const int32_t *col_gid, uint64_t seed, const int64_t *step,
                                          int32_t layer, uint32_t thr, pgcn_stream_t stream) {
    const Stats rc{reinterpret_cast<const float4 *>(rowstat), s2, lds2, nrows, slope};
    const EdgeGrad eg{Z, ldz, t, heads * d + (heads + 3) / 4 * 4};
    const Mask mk{row_gid, col_gid, seed, step, (uint64_t)(layer < 0 ? 0 : layer), thr, dropout_scale(thr)};
    return launch_attndrop("pgcn_gat_attndrop_grad_f32", rowptr, col, rc, &eg, nullptr, mk, layer, heads, d, nrows, tasks, ntasks, seg,
                           nslices, fix, nfix, B, ldb, C, ldc, partial_ws, partial_ws_elems, nslots, flags, stream);
}
