// pgcn_aggpna.hip -- the four aggregators of Principal Neighbourhood Aggregation (Corso et al., NeurIPS 2020; PyG's PNAConv) in ONE
// gather for gfx950 (MI355X / CDNA4), fp32, their backward, and the degree scalers.  cand(i) = the stored columns of row i (values
// ignored), d_i = |cand(i)| over ALL the structures that hold a piece of row i, x_j = B[j, c]:
//
//   MEAN[i, c] = (1 / d_i) sum_j x_j
//   MAX / AMAX   pgcn_aggmax.hip's definition and tie rule (the smallest GLOBAL id among the maxima, fp32 ==)
//   MIN / AMIN   the mirror image: (v, g) replaces (cur, a) when a < 0 || v < cur || (v == cur && g < a)
//   VAR[i, c]  = (1 / d_i) sum_j (x_j - MEAN[i, c])^2        STD = sqrt(VAR + 1e-5f)
//   d_i = 0: all four 0.0f, AMAX = AMIN = -1                 S[i, :] = [MEAN | MAX | MIN | STD]   (n x 4 f)
//
// The variance is NOT E[x^2] - E[x]^2 (that cancels on rows of equal values and on a common offset).  A group of candidates is the
// mergeable state (cnt, mean, M2), M2 = sum (x - mean)^2:
//   * inside a task a lane keeps shifted sums around the task's first value K: s1 = sum (x - K), s2 = sum (x - K)^2 -- one subtract and
//     two FMAs per element -- and closes with mean = K + s1 / cnt, M2 = max(s2 - s1 s1 / cnt, 0);
//   * two groups merge by Chan's rule: dl = m_b - m_a, mean = m_a + dl n_b / n, M2 = M2_a + M2_b + dl^2 n_a n_b / n.  The one rule merges
//     the pieces of a cut row (the fix-up, in slot order) and, under PGCN_SPMM_ACCUMULATE, the row's current state with a call's result;
//   * while structures are still to come the fourth block of S holds M2; finish_kernel turns it into STD once, after the last one.
// Equal values give M2 = 0 exactly (every x - K is 0); an offset of 10^3 on every value costs no digits.
// The count of a row is ONE int32 per row, not one per feature: cnt_prior[i] = the candidates already merged into row i's state (read
// under PGCN_SPMM_ACCUMULATE only; this call's own count is the task length), so the feature passes of a row never write a shared word.
//
// Mapping to the machine: the work decomposition of aggmax_tasks_kernel -- LPR lanes per task, VEC consecutive features per lane, the
// (col, gid) pair stream loaded coalesced and non-temporal and parked in the wave's LDS, eight row loads in flight per batch, the
// unsliced or the XCD-sliced plan, 64-feature passes.  Per feature a lane holds K, s1, s2, max, amax, min, amin: 28 registers at VEC = 4
// beside the 32 of the loads in flight.  Inside a task the pairs ascend by global id, so an equal value never replaces: the max and the
// min cost one compare and two selects each.  The loads of a ragged batch are NOT predicated: the surplus slots re-read the task's last
// row and are selected out.  Pieces of a cut row go to six planes of the work-space (mean, M2, max, min, amax, amin: nslots x f each)
// and one int32 count per slot behind them.
//
// Backward.  dS = [dMEAN | dMAX | dMIN | dSTD]; finish_kernel forms, per row i, Q = dSTD / (d STD), P = dMEAN / d - Q MEAN and writes
// the PANEL: row i holds six planes of fp = 4 ceil(f / 4) words, {P | Q | dMAX | dMIN | AMAX | AMIN} at panel[i * ldp + k fp], ldp = 6 fp
// -- the operands of a stored entry are ONE contiguous region of 6 fp x 4 bytes, and every load instruction of a group still reads one
// dense segment of a plane.  (Interleaving the six per quad of features was measured first: the lanes of a load then sit 96 bytes apart,
// six times the cache lines per instruction, and the backward ran 1.19 x the four launches it replaces.)  An entry reads P, Q, AMAX and
// AMIN; dMAX and dMIN are fetched only by the lanes whose row holds a winning id -- a row wins 1 / d of its neighbours' extremes.  Over
// the transposed structure, row r with global id g_r and its own features X[r, :]:
//   D[r, c] = sum_i ( P[i, c] + (AMAX[i, c] == g_r ? dMAX[i, c] : 0) + (AMIN[i, c] == g_r ? dMIN[i, c] : 0) ) + X[r, c] sum_i Q[i, c]
// -- gather form, entries in storage order, no atomics.  The X sum Q term is applied per piece, so a cut row needs one partial plane and
// pgcn_spmm_fixup_f32 adds the pieces in slot order.
//
// The scalers and the finishing kernel use the row-band layout of pgcn_rowband.h.  Inputs are finite by contract.  Plain vector loads
// and stores only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_device.h"
#include "pgcn_internal.h"
#include "pgcn_rowband.h"

namespace {

constexpr int kWavesPerBlock = 4;
static_assert(kThreads == kWavesPerBlock * 64, "the gather kernels run the row-band block size");
constexpr int kUnrollFwd = 8;   // row loads of B in flight per batch
constexpr int kUnrollBwd = 4;   // entries per batch of the backward: four panel vectors each (P, Q, AMAX, AMIN) = sixteen loads
constexpr int kPanelQuad = 24;  // words of a panel row per quad of features: six planes
constexpr float kEps = 1e-5f;

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

template <bool OFF32>
__device__ __forceinline__ const float *row_at(const float *base, uint32_t lane_byte_off, int32_t c, int64_t ld) {
    if constexpr (OFF32) {
        return reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + ((uint32_t)c * (uint32_t)(ld * 4) + lane_byte_off));
    } else {
        return reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + ((int64_t)c * ld * 4 + lane_byte_off));
    }
}

// the order rules between finished groups; `ok`: the candidate exists (a slot or a row that holds an arg)
__device__ __forceinline__ void take_max(float &cur, int32_t &arg, float v, int32_t g, bool ok) {
    const bool take = ok && (arg < 0 || v > cur || (v == cur && g < arg));
    cur = take ? v : cur;
    arg = take ? g : arg;
}

__device__ __forceinline__ void take_min(float &cur, int32_t &arg, float v, int32_t g, bool ok) {
    const bool take = ok && (arg < 0 || v < cur || (v == cur && g < arg));
    cur = take ? v : cur;
    arg = take ? g : arg;
}

// Chan's rule: the group (nb, mb, Mb) joins the state (na, ma, Ma); a count of 0: absent
__device__ __forceinline__ void merge_var(float na, float &ma, float &Ma, float nb, float mb, float Mb) {
    if (nb == 0.f) return;
    if (na == 0.f) { ma = mb; Ma = Mb; return; }
    const float r = nb / (na + nb);
    const float dl = mb - ma;
    ma = fmaf(dl, r, ma);
    Ma = fmaf(dl * dl, na * r, Ma + Mb);
}

struct Task { int64_t kbeg; int32_t len, dst; };

struct SliceSeg { int64_t v[PGCN_MAX_SLICES + 1]; };

// the planes of the pieces of cut rows: nslots x f each, and one count per slot
struct Planes { float *mean, *m2, *mx, *mn; int32_t *amx, *amn, *cnt; };

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
// S: [MEAN | MAX | MIN | M2] at columns 0, f, 2 f, 3 f of a row of leading dimension lds
template <int LPR, int VEC, bool OFF32>
__global__ __launch_bounds__(kThreads, 4) void aggpna_tasks_kernel(
    const int64_t *__restrict__ rowptr, const uint64_t *__restrict__ pairs, const int4 *__restrict__ tasks, int64_t ntasks,
    const float *__restrict__ B, int64_t ldb, float *__restrict__ S, int64_t lds, int32_t *__restrict__ AMAX, int64_t ldx,
    int32_t *__restrict__ AMIN, int64_t ldn, const int32_t *__restrict__ cnt_prior, int32_t f, Planes pl, int64_t nblocks,
    uint32_t flags, int32_t nslices, SliceSeg seg) {
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

    float K[VEC], s1[VEC], s2[VEC], mx[VEC], mn[VEC];
    int32_t amx[VEC], amn[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { K[v] = 0.f; s1[v] = 0.f; s2[v] = 0.f; mx[v] = 0.f; mn[v] = 0.f; amx[v] = -1; amn[v] = -1; }
    bool none = true;   // no entry of this task taken yet: the first one sets K, the max and the min

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
                for (int u = 0; u < U; ++u) vload<VEC>(x[u], row_at<OFF32>(B, lane_off, c[u], ldb));
#pragma unroll
                for (int u = 0; u < U; ++u) {   // ascending global ids inside a task: an equal value never replaces
                    const bool ok = k + u < cnt;
                    const bool first = ok && none;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float xv = x[u][v];
                        K[v] = first ? xv : K[v];
                        const float dl = ok ? xv - K[v] : 0.f;
                        s1[v] += dl;
                        s2[v] = fmaf(dl, dl, s2[v]);
                        const bool up = first || (ok && xv > mx[v]);
                        mx[v] = up ? xv : mx[v];
                        amx[v] = up ? g[u] : amx[v];
                        const bool dn = first || (ok && xv < mn[v]);
                        mn[v] = dn ? xv : mn[v];
                        amn[v] = dn ? g[u] : amn[v];
                    }
                    none = none && !ok;
                }
            }
        }
    }

    if (tact && fact) {
        const float n = (float)(len > 0 ? len : 1);
        float mean[VEC], m2[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float q = s1[v] / n;
            mean[v] = K[v] + q;
            m2[v] = fmaxf(fmaf(-s1[v], q, s2[v]), 0.f);
        }
        if (t.dst >= 0) {
            const int64_t o = (int64_t)t.dst * f + fcol;
            vstore<VEC>(pl.mean + o, mean);
            vstore<VEC>(pl.m2 + o, m2);
            vstore<VEC>(pl.mx + o, mx);
            vstore<VEC>(pl.mn + o, mn);
            istore<VEC>(pl.amx + o, amx);
            istore<VEC>(pl.amn + o, amn);
            if (blockIdx.y == 0 && sub == 0) pl.cnt[t.dst] = len;
        } else {
            const int64_t row = ~t.dst;
            float *s = S + row * lds + fcol;
            int32_t *ax = AMAX + row * ldx + fcol;
            int32_t *an = AMIN + row * ldn + fcol;
            if (flags & PGCN_SPMM_ACCUMULATE) {   // the row's current state takes this task's result as one more group
                const float na = (float)cnt_prior[row];
                float cm[VEC], c2[VEC], cx[VEC], cn[VEC];
                int32_t cax[VEC], can[VEC];
                vload<VEC>(cm, s);
                vload<VEC>(cx, s + f);
                vload<VEC>(cn, s + 2 * (int64_t)f);
                vload<VEC>(c2, s + 3 * (int64_t)f);
                iload<VEC>(cax, ax);
                iload<VEC>(can, an);
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    merge_var(na, cm[v], c2[v], (float)len, mean[v], m2[v]);
                    take_max(cx[v], cax[v], mx[v], amx[v], amx[v] >= 0);
                    take_min(cn[v], can[v], mn[v], amn[v], amn[v] >= 0);
                    mean[v] = cm[v]; m2[v] = c2[v]; mx[v] = cx[v]; mn[v] = cn[v]; amx[v] = cax[v]; amn[v] = can[v];
                }
            }
            vstore<VEC>(s, mean);
            vstore<VEC>(s + f, mx);
            vstore<VEC>(s + 2 * (int64_t)f, mn);
            vstore<VEC>(s + 3 * (int64_t)f, m2);
            istore<VEC>(ax, amx);
            istore<VEC>(an, amn);
        }
    }
}

// fix: int4 {row, first slot, #slots, unused}: merges the slots of a cut row in slot order by the three rules
template <int LPR, int VEC>
__global__ __launch_bounds__(kThreads) void aggpna_fixup_kernel(
    const int4 *__restrict__ fix, int64_t nfix, Planes pl, float *__restrict__ S, int64_t lds, int32_t *__restrict__ AMAX, int64_t ldx,
    int32_t *__restrict__ AMIN, int64_t ldn, const int32_t *__restrict__ cnt_prior, int32_t f, uint32_t flags) {
    constexpr int G = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t id = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * G + lane / LPR;
    const int fcol = (blockIdx.y * LPR + lane % LPR) * VEC;
    if (id >= nfix || fcol >= f) return;
    const int4 t = fix[id];
    float *s = S + (int64_t)t.x * lds + fcol;
    int32_t *ax = AMAX + (int64_t)t.x * ldx + fcol;
    int32_t *an = AMIN + (int64_t)t.x * ldn + fcol;
    float n = 0.f, mean[VEC], m2[VEC], mx[VEC], mn[VEC];
    int32_t amx[VEC], amn[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { mean[v] = 0.f; m2[v] = 0.f; mx[v] = 0.f; mn[v] = 0.f; amx[v] = -1; amn[v] = -1; }
    if (flags & PGCN_SPMM_ACCUMULATE) {
        n = (float)cnt_prior[t.x];
        vload<VEC>(mean, s);
        vload<VEC>(mx, s + f);
        vload<VEC>(mn, s + 2 * (int64_t)f);
        vload<VEC>(m2, s + 3 * (int64_t)f);
        iload<VEC>(amx, ax);
        iload<VEC>(amn, an);
    }
    for (int sl = 0; sl < t.z; ++sl) {
        const int64_t o = (int64_t)(t.y + sl) * f + fcol;
        const float nb = (float)pl.cnt[t.y + sl];
        float bm[VEC], b2[VEC], bx[VEC], bn[VEC];
        int32_t bax[VEC], ban[VEC];
        vload<VEC>(bm, pl.mean + o);
        vload<VEC>(b2, pl.m2 + o);
        vload<VEC>(bx, pl.mx + o);
        vload<VEC>(bn, pl.mn + o);
        iload<VEC>(bax, pl.amx + o);
        iload<VEC>(ban, pl.amn + o);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            merge_var(n, mean[v], m2[v], nb, bm[v], b2[v]);
            take_max(mx[v], amx[v], bx[v], bax[v], bax[v] >= 0);
            take_min(mn[v], amn[v], bn[v], ban[v], ban[v] >= 0);
        }
        n += nb;
    }
    vstore<VEC>(s, mean);
    vstore<VEC>(s + f, mx);
    vstore<VEC>(s + 2 * (int64_t)f, mn);
    vstore<VEC>(s + 3 * (int64_t)f, m2);
    istore<VEC>(ax, amx);
    istore<VEC>(an, amn);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The finishing kernel, row-band layout.  BWD false: S's fourth block M2 -> STD in place.  BWD true: the panel of the backward.
__device__ __forceinline__ Quad as_float(const int32_t *row, int c0, int f, bool vec) {
    Quad q;
    if (vec) {
        const int4 t = *reinterpret_cast<const int4 *>(row + c0);
        q.v[0] = __int_as_float(t.x), q.v[1] = __int_as_float(t.y), q.v[2] = __int_as_float(t.z), q.v[3] = __int_as_float(t.w);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) q.v[j] = __int_as_float(c0 + j < f ? row[c0 + j] : -1);
    }
    return q;
}

template <bool VEC, bool BWD>
__global__ __launch_bounds__(kThreads) void finish_kernel(float *S, int64_t lds, const int32_t *__restrict__ deg, int64_t nrows, int f,
                                                          int log2_tpr, const float *__restrict__ dS, int64_t ldds,
                                                          const int32_t *__restrict__ AMAX, int64_t ldx,
                                                          const int32_t *__restrict__ AMIN, int64_t ldn, float *__restrict__ panel,
                                                          int64_t ldp, bool ivec) {
    const Band b = band_of(log2_tpr, kApplyRows, nrows);
    if (b.c0 >= f) return;
    for (int64_t r = b.r0 + b.rg; r < b.rend; r += b.ngroups) {
        const int32_t d = deg[r];
        const float dn = (float)(d > 0 ? d : 1);
        float *s = S + r * lds;
        if constexpr (!BWD) {
            Quad m2 = load_quad<VEC>(s + 3 * (int64_t)f, b.c0, f);
#pragma unroll
            for (int j = 0; j < 4; ++j) m2.v[j] = d > 0 ? sqrtf(m2.v[j] / dn + kEps) : 0.f;
            store_quad<VEC>(s + 3 * (int64_t)f, b.c0, f, m2);
        } else {
            const float *g = dS + r * ldds;
            const Quad mean = load_quad<VEC>(s, b.c0, f), sd = load_quad<VEC>(s + 3 * (int64_t)f, b.c0, f);
            const Quad gm = load_quad<VEC>(g, b.c0, f), gsd = load_quad<VEC>(g + 3 * (int64_t)f, b.c0, f);
            Quad P, Q;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                Q.v[j] = d > 0 && sd.v[j] > 0.f ? gsd.v[j] / (dn * sd.v[j]) : 0.f;      // (STD >= sqrt(1e-5) wherever d > 0; 0 beyond f)
                P.v[j] = d > 0 ? fmaf(-Q.v[j], mean.v[j], gm.v[j] / dn) : 0.f;
            }
            const int fp = (f + 3) & ~3;                               // (the planes are whole quads: float4 stores, zeros and -1 beyond f)
            float *p = panel + r * ldp + b.c0;
            store_quad<true>(p, 0, fp, P);
            store_quad<true>(p, fp, 2 * fp, Q);
            store_quad<true>(p, 2 * fp, 3 * fp, load_quad<VEC>(g + f, b.c0, f));
            store_quad<true>(p, 3 * fp, 4 * fp, load_quad<VEC>(g + 2 * (int64_t)f, b.c0, f));
            store_quad<true>(p, 4 * fp, 5 * fp, as_float(AMAX + r * ldx, b.c0, f, ivec));
            store_quad<true>(p, 5 * fp, 6 * fp, as_float(AMIN + r * ldn, b.c0, f, ivec));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Backward over the transposed structure: task rows are rows of D and of X, stored entries index the rows of the panel.
template <int LPR, int VEC, bool OFF32>
__global__ __launch_bounds__(kThreads, 4) void aggpna_backward_tasks_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int4 *__restrict__ tasks, int64_t ntasks,
    const int32_t *__restrict__ rowgid, const int32_t *__restrict__ slot_row, const float *__restrict__ X, int64_t ldx,
    const float *__restrict__ panel, int64_t ldp, float *__restrict__ D, int64_t ldd, int32_t f, float *__restrict__ partial,
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
    const uint32_t lane_off = (uint32_t)fcol * 4u;   // this lane's first word inside every plane of a panel row
    const int fp = (f + 3) & ~3;                     // words of a plane

    float acc[VEC], qs[VEC], xr[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { acc[v] = 0.f; qs[v] = 0.f; xr[v] = 0.f; }
    int32_t gid = -2;   // (-2: no task; the panel holds ids >= 0 or -1, so nothing matches)
    if (tact) {
        const int64_t r = t.dst >= 0 ? slot_row[t.dst] : ~t.dst;
        gid = rowgid[r];
        if (fact) vload<VEC>(xr, X + r * ldx + fcol);   // this task's own row of X
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
            float w[U][4][VEC];   // P, Q, AMAX, AMIN of the entry; dMAX / dMIN are fetched only by the lanes whose row won
            const float *pe[U];
#pragma unroll
            for (int u = 0; u < U; ++u) c[u] = mg[k + u];
            if (fact) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    pe[u] = row_at<OFF32>(panel, lane_off, c[u], ldp);
                    vload<VEC>(w[u][0], pe[u]);
                    vload<VEC>(w[u][1], pe[u] + fp);
                    vload<VEC>(w[u][2], pe[u] + 4 * fp);
                    vload<VEC>(w[u][3], pe[u] + 5 * fp);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool ok = k + u < cnt;
                    // a row wins 1 / d of the extremes of its neighbours: the two gradient vectors (a third of the panel) are read
                    // by the few lanes that hold a match, after the ids arrived
                    bool hx = false, hn = false;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        hx = hx || __float_as_int(w[u][2][v]) == gid;
                        hn = hn || __float_as_int(w[u][3][v]) == gid;
                    }
                    float gx[VEC], gn[VEC];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) { gx[v] = 0.f; gn[v] = 0.f; }
                    if (ok && hx) vload<VEC>(gx, pe[u] + 2 * fp);
                    if (ok && hn) vload<VEC>(gn, pe[u] + 3 * fp);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        float e = w[u][0][v];
                        e += (__float_as_int(w[u][2][v]) == gid) ? gx[v] : 0.f;
                        e += (__float_as_int(w[u][3][v]) == gid) ? gn[v] : 0.f;
                        acc[v] += ok ? e : 0.f;
                        qs[v] += ok ? w[u][1][v] : 0.f;
                    }
                }
            }
        }
    }

    if (tact && fact) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = fmaf(xr[v], qs[v], acc[v]);
        if (t.dst >= 0) vstore<VEC>(partial + (int64_t)t.dst * f + fcol, acc);
        else vstore<VEC>(D + (int64_t)(~t.dst) * ldd + fcol, acc);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The degree scalers, row-band layout.  Y = [Y0 | Y1 | Y2] (n x 3 fo):  Z = Y0 + a Y1 + b Y2;  backward dY = [G | a G | b G].
template <bool VEC>
__global__ __launch_bounds__(kThreads) void scale_forward_kernel(const float *__restrict__ Y, int64_t ldy, const float *__restrict__ a,
                                                                 const float *__restrict__ bsc, float *__restrict__ Z, int64_t ldz,
                                                                 int64_t nrows, int fo, int log2_tpr) {
    const Band b = band_of(log2_tpr, kApplyRows, nrows);
    if (b.c0 >= fo) return;
    for (int64_t r = b.r0 + b.rg; r < b.rend; r += b.ngroups) {
        const float *y = Y + r * ldy;
        const float ar = a[r], br = bsc[r];
        const Quad y0 = load_quad<VEC>(y, b.c0, fo), y1 = load_quad<VEC>(y + fo, b.c0, fo), y2 = load_quad<VEC>(y + 2 * (int64_t)fo, b.c0, fo);
        Quad z;
#pragma unroll
        for (int j = 0; j < 4; ++j) z.v[j] = fmaf(br, y2.v[j], fmaf(ar, y1.v[j], y0.v[j]));
        store_quad<VEC>(Z + r * ldz, b.c0, fo, z);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void scale_backward_kernel(const float *__restrict__ G, int64_t ldg, const float *__restrict__ a,
                                                                  const float *__restrict__ bsc, float *__restrict__ dY, int64_t ldy,
                                                                  int64_t nrows, int fo, int log2_tpr) {
    const Band b = band_of(log2_tpr, kApplyRows, nrows);
    if (b.c0 >= fo) return;
    for (int64_t r = b.r0 + b.rg; r < b.rend; r += b.ngroups) {
        float *y = dY + r * ldy;
        const float ar = a[r], br = bsc[r];
        const Quad g = load_quad<VEC>(G + r * ldg, b.c0, fo);
        Quad g1, g2;
#pragma unroll
        for (int j = 0; j < 4; ++j) { g1.v[j] = ar * g.v[j]; g2.v[j] = br * g.v[j]; }
        store_quad<VEC>(y, b.c0, fo, g);
        store_quad<VEC>(y + fo, b.c0, fo, g1);
        store_quad<VEC>(y + 2 * (int64_t)fo, b.c0, fo, g2);
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
                   int32_t nslices, const int32_t *fix, int64_t nfix, const float *B, int64_t ldb, float *S, int64_t lds, int32_t *AMAX,
                   int64_t ldx, int32_t *AMIN, int64_t ldn, const int32_t *cnt_prior, int32_t f, Planes pl, uint32_t flags,
                   hipStream_t s) {
    SliceSeg seg{};
    const Grid g = task_grid<LPR, VEC>(ntasks, f, flags, nslices, seg_host, seg);
    if (g.blocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_csr_plan_f32: too many tasks for one launch");
    const uint64_t *p64 = reinterpret_cast<const uint64_t *>(pairs);
    const int4 *t4 = reinterpret_cast<const int4 *>(tasks);
    if (flags & PGCN_SPMM_OFFSETS32)
        hipLaunchKernelGGL((aggpna_tasks_kernel<LPR, VEC, true>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s, rowptr, p64,
                           t4, ntasks, B, ldb, S, lds, AMAX, ldx, AMIN, ldn, cnt_prior, f, pl, g.blocks, flags, nslices, seg);
    else
        hipLaunchKernelGGL((aggpna_tasks_kernel<LPR, VEC, false>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s, rowptr, p64,
                           t4, ntasks, B, ldb, S, lds, AMAX, ldx, AMIN, ldn, cnt_prior, f, pl, g.blocks, flags, nslices, seg);
    PGCN_HIP_CHECK(hipGetLastError());
    if (nfix > 0) {
        const int64_t per_block = (int64_t)kWavesPerBlock * (64 / LPR);
        hipLaunchKernelGGL((aggpna_fixup_kernel<LPR, VEC>), dim3((unsigned)((nfix + per_block - 1) / per_block), g.ntiles),
                           dim3(kThreads), 0, s, reinterpret_cast<const int4 *>(fix), nfix, pl, S, lds, AMAX, ldx, AMIN, ldn, cnt_prior, f,
                           flags);
        PGCN_HIP_CHECK(hipGetLastError());
    }
    return PGCN_OK;
}

template <int LPR, int VEC>
int launch_backward(const int64_t *rowptr, const int32_t *col, const int32_t *tasks, int64_t ntasks, const int64_t *seg_host,
                    int32_t nslices, const int32_t *rowgid, const int32_t *slot_row, const float *X, int64_t ldx, const float *panel,
                    int64_t ldp, float *D, int64_t ldd, int32_t f, float *partial, uint32_t flags, hipStream_t s) {
    SliceSeg seg{};
    const Grid g = task_grid<LPR, VEC>(ntasks, f, flags, nslices, seg_host, seg);
    if (g.blocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_backward_csr_plan_f32: too many tasks for one launch");
    const int4 *t4 = reinterpret_cast<const int4 *>(tasks);
    if (flags & PGCN_SPMM_OFFSETS32)
        hipLaunchKernelGGL((aggpna_backward_tasks_kernel<LPR, VEC, true>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s,
                           rowptr, col, t4, ntasks, rowgid, slot_row, X, ldx, panel, ldp, D, ldd, f, partial, g.blocks, flags, nslices,
                           seg);
    else
        hipLaunchKernelGGL((aggpna_backward_tasks_kernel<LPR, VEC, false>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s,
                           rowptr, col, t4, ntasks, rowgid, slot_row, X, ldx, panel, ldp, D, ldd, f, partial, g.blocks, flags, nslices,
                           seg);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

}  // namespace

#define PGCN_AGGPNA_SHAPES(CASE)                                                           \
    CASE(1, 4) CASE(2, 4) CASE(4, 4) CASE(8, 4) CASE(16, 4) CASE(32, 4) CASE(64, 4)        \
    CASE(1, 1) CASE(2, 1) CASE(4, 1) CASE(8, 1) CASE(16, 1) CASE(32, 1) CASE(64, 1)

extern "C" int pgcn_aggpna_csr_plan_f32(const int64_t *rowptr, const int32_t *pairs, const int32_t *tasks, int64_t ntasks,
                                        const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const float *B,
                                        int64_t ldb, float *S, int64_t lds, int32_t *AMAX, int64_t ldx, int32_t *AMIN, int64_t ldn,
                                        const int32_t *cnt_prior, int32_t f, void *ws, int64_t ws_bytes, int64_t nslots, uint32_t flags,
                                        pgcn_stream_t stream) {
    if (ntasks < 0 || nfix < 0 || nslots < 0 || f < 1 || ldb < f || lds < 4 * (int64_t)f || ldx < f || ldn < f || nslices < 1 ||
        nslices > PGCN_MAX_SLICES || (nslices > 1 && (!seg || !tasks)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_csr_plan_f32: bad sizes");
    if (nslices > 1 && (seg[0] != 0 || seg[nslices] != ntasks))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_csr_plan_f32: seg does not cover the task list");
    if (ntasks == 0) return PGCN_OK;
    if (!rowptr || !pairs || !B || !S || !AMAX || !AMIN || (nfix > 0 && (!fix || !tasks)) || (nslots > 0 && !ws) ||
        ((flags & PGCN_SPMM_ACCUMULATE) && !cnt_prior))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_csr_plan_f32: null pointer");
    if (ntasks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_csr_plan_f32: ntasks >= 2^31");
    if ((uintptr_t)pairs % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_csr_plan_f32: pairs must be 8-byte aligned");
    const int64_t plane = nslots * (int64_t)f;
    if (ws_bytes < plane * 24 + nslots * 4) return pgcn_set_error(PGCN_ENOMEM, "pgcn_aggpna_csr_plan_f32: work-space too small");
    if ((uintptr_t)ws % 4 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_csr_plan_f32: ws must be 4-byte aligned");
    float *w = reinterpret_cast<float *>(ws);                    // mean, M2, max, min, amax, amin: nslots x f each; then nslots counts
    int32_t *wi = reinterpret_cast<int32_t *>(ws);
    const Planes pl{w, w + plane, w + 2 * plane, w + 3 * plane, wi + 4 * plane, wi + 5 * plane, wi + 6 * plane};
    // (f % 4 == 0: every plane starts a multiple of 16 bytes behind ws, every block of S a multiple of 16 bytes behind its row)
    const Shape sh = pick_shape(f, aligned16(B) && aligned16(S) && aligned16(AMAX) && aligned16(AMIN) && aligned16(ws) && rows16(ldb) &&
                                       rows16(lds) && rows16(ldx) && rows16(ldn) && f % 4 == 0, flags);
#define PGCN_CASE(L, V)                                                                                                                \
    if (sh.lpr == L && sh.vec == V)                                                                                                    \
        return launch_forward<L, V>(rowptr, pairs, tasks, ntasks, seg, nslices, fix, nfix, B, ldb, S, lds, AMAX, ldx, AMIN, ldn, cnt_prior, \
                                    f, pl, flags, (hipStream_t)stream);
    PGCN_AGGPNA_SHAPES(PGCN_CASE)
#undef PGCN_CASE
    return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_csr_plan_f32: no kernel shape");
}

extern "C" int pgcn_aggpna_finish_f32(float *S, int64_t lds, const int32_t *deg, int64_t nrows, int32_t f, const float *dS, int64_t ldds,
                                      const int32_t *AMAX, int64_t ldx, const int32_t *AMIN, int64_t ldn, float *panel, int64_t ldp,
                                      pgcn_stream_t stream) {
    const bool bwd = dS != nullptr;
    if (nrows < 0 || f < 1 || f > kMaxF || lds < 4 * (int64_t)f)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_finish_f32: bad sizes (1 <= f <= 1024, lds >= 4 f)");
    if (bwd && (ldds < 4 * (int64_t)f || ldx < f || ldn < f || ldp < kPanelQuad * (((int64_t)f + 3) / 4)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_finish_f32: a leading dimension is too small (ldp >= 24 ceil(f / 4))");
    if (nrows == 0) return PGCN_OK;
    if (!S || !deg || (bwd && (!AMAX || !AMIN || !panel))) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_finish_f32: null pointer");
    if (bwd && (!aligned16(panel) || !rows16(ldp)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_finish_f32: the panel and its rows must be 16-byte aligned");
    const int64_t nblocks = apply_blocks(nrows);
    if (nblocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_finish_f32: too many rows");
    const int l2 = log2_threads_per_row(f);
    const bool vec = f % 4 == 0 && rows16(lds) && aligned16(S) && (!bwd || (rows16(ldds) && aligned16(dS)));
    const bool ivec = bwd && f % 4 == 0 && rows16(ldx) && rows16(ldn) && aligned16(AMAX) && aligned16(AMIN);
    hipStream_t s = (hipStream_t)stream;
    if (bwd)
        launch(vec ? finish_kernel<true, true> : finish_kernel<false, true>, nblocks, s, S, lds, deg, nrows, f, l2, dS, ldds, AMAX, ldx,
               AMIN, ldn, panel, ldp, ivec);
    else
        launch(vec ? finish_kernel<true, false> : finish_kernel<false, false>, nblocks, s, S, lds, deg, nrows, f, l2, dS, ldds, AMAX, ldx,
               AMIN, ldn, panel, ldp, ivec);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_aggpna_backward_csr_plan_f32(const int64_t *rowptr, const int32_t *col, const int32_t *rowgid,
                                                 const int32_t *slot_row, const int32_t *tasks, int64_t ntasks, const int64_t *seg,
                                                 int32_t nslices, const int32_t *fix, int64_t nfix, const float *X, int64_t ldx,
                                                 const float *panel, int64_t ldp, float *D, int64_t ldd, int32_t f, float *partial_ws,
                                                 int64_t partial_ws_elems, int64_t nslots, uint32_t flags, pgcn_stream_t stream) {
    if (ntasks < 0 || nfix < 0 || nslots < 0 || f < 1 || ldx < f || ldd < f || ldp < kPanelQuad * (((int64_t)f + 3) / 4) || nslices < 1 ||
        nslices > PGCN_MAX_SLICES || (nslices > 1 && (!seg || !tasks)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_backward_csr_plan_f32: bad sizes");
    if (nslices > 1 && (seg[0] != 0 || seg[nslices] != ntasks))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_backward_csr_plan_f32: seg does not cover the task list");
    if (ntasks == 0) return PGCN_OK;
    if (!rowptr || !col || !rowgid || !X || !panel || !D || (nfix > 0 && (!fix || !tasks)) || (nslots > 0 && (!partial_ws || !slot_row)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_backward_csr_plan_f32: null pointer");
    if (ntasks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_backward_csr_plan_f32: ntasks >= 2^31");
    if (!aligned16(panel) || !rows16(ldp))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_backward_csr_plan_f32: the panel and its rows must be 16-byte aligned");
    if (partial_ws_elems < nslots * (int64_t)f)
        return pgcn_set_error(PGCN_ENOMEM, "pgcn_aggpna_backward_csr_plan_f32: partial work-space too small");
    const Shape sh = pick_shape(f, aligned16(X) && aligned16(D) && aligned16(partial_ws) && rows16(ldx) && rows16(ldd) && f % 4 == 0, flags);
    int rc = 1;   // (no shape taken yet)
#define PGCN_CASE(L, V)                                                                                                                 \
    if (sh.lpr == L && sh.vec == V)                                                                                                     \
        rc = launch_backward<L, V>(rowptr, col, tasks, ntasks, seg, nslices, rowgid, slot_row, X, ldx, panel, ldp, D, ldd, f, partial_ws, \
                                   flags, (hipStream_t)stream);
    PGCN_AGGPNA_SHAPES(PGCN_CASE)
#undef PGCN_CASE
    if (rc == 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_aggpna_backward_csr_plan_f32: no kernel shape");
    if (rc != PGCN_OK || nfix == 0) return rc;
    // the pieces of a cut row, added in slot order (the sum path's fix-up: the slots hold plain partial sums)
    return pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_ws, D, ldd, f, 0u, stream);
}

extern "C" int pgcn_pna_scale_forward_f32(const float *Y, int64_t ldy, const float *a, const float *b, float *Z, int64_t ldz,
                                          int64_t nrows, int32_t fout, pgcn_stream_t stream) {
    if (nrows < 0 || fout < 1 || fout > kMaxF || ldy < 3 * (int64_t)fout || ldz < fout)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_pna_scale_forward_f32: bad sizes (1 <= fout <= 1024, ldy >= 3 fout, ldz >= fout)");
    if (nrows == 0) return PGCN_OK;
    if (!Y || !a || !b || !Z) return pgcn_set_error(PGCN_EINVAL, "pgcn_pna_scale_forward_f32: null pointer");
    const int64_t nblocks = apply_blocks(nrows);
    if (nblocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_pna_scale_forward_f32: too many rows");
    const bool vec = fout % 4 == 0 && rows16(ldy) && rows16(ldz) && aligned16(Y) && aligned16(Z);
    launch(vec ? scale_forward_kernel<true> : scale_forward_kernel<false>, nblocks, (hipStream_t)stream, Y, ldy, a, b, Z, ldz, nrows,
           fout, log2_threads_per_row(fout));
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_pna_scale_backward_f32(const float *G, int64_t ldg, const float *a, const float *b, float *dY, int64_t ldy,
                                           int64_t nrows, int32_t fout, pgcn_stream_t stream) {
    if (nrows < 0 || fout < 1 || fout > kMaxF || ldy < 3 * (int64_t)fout || ldg < fout)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_pna_scale_backward_f32: bad sizes (1 <= fout <= 1024, ldy >= 3 fout, ldg >= fout)");
    if (nrows == 0) return PGCN_OK;
    if (!G || !a || !b || !dY) return pgcn_set_error(PGCN_EINVAL, "pgcn_pna_scale_backward_f32: null pointer");
    const int64_t nblocks = apply_blocks(nrows);
    if (nblocks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_pna_scale_backward_f32: too many rows");
    const bool vec = fout % 4 == 0 && rows16(ldy) && rows16(ldg) && aligned16(G) && aligned16(dY);
    launch(vec ? scale_backward_kernel<true> : scale_backward_kernel<false>, nblocks, (hipStream_t)stream, G, ldg, a, b, dY, ldy, nrows,
           fout, log2_threads_per_row(fout));
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}
