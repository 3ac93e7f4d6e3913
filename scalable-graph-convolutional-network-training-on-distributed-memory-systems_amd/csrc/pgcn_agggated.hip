// pgcn_agggated.hip -- GATED aggregation over the neighbourhood (GatedGCN, Bresson & Laurent 2017; Dwivedi et al., "Benchmarking GNNs")
// for gfx950 (MI355X / CDNA4), fp32, and its backward.  A gate PER FEATURE column c that depends on BOTH ends of a stored entry (i, j)
// (stored values ignored), K / Q / V the key, query and value projections of the vertices:
//
//   g_ij,c    = 1 / (1 + exp(-(K[i, c] + Q[j, c])))                      the argument clamped to [-80, 80] (g and 1 - g stay normal numbers)
//   NUM[i, c] = sum_j g_ij,c V[j, c]      DEN[i, c] = sum_j g_ij,c      Z1 = NUM / (DEN + 1e-6f)        a row without entries: 0.0f
//   backward, G = dZ1, P_i = G_i / (DEN_i + 1e-6f), O_i = Z1_i:
//   t_ij = P_i (V_j - O_i) g_ij (1 - g_ij)      dK_i = sum_j t_ij      dQ_j = sum_i t_ij      dV_j = sum_i g_ij P_i
//
// The n x nnz x f gates are never stored: every kernel recomputes them inside its gather from e = exp(-(k + q)), g = 1 / (1 + e) and
// 1 - g = e g (a product, not a difference: a gate that rounds to 1 keeps its slope).  (NUM, DEN) is an ADDITIVE state: the pieces of a
// cut row add up in slot order through pgcn_spmm_fixup_f32, PGCN_SPMM_ACCUMULATE adds a structure's result to what the rows hold -- no
// merge rule, no atomics.
//
// Mapping to the machine: the work decomposition of aggmax_tasks_kernel (pgcn_aggmax.hip) -- LPR lanes per task, VEC consecutive
// features per lane, the entry stream loaded coalesced and non-temporal and parked in the wave's LDS, the unsliced or the XCD-sliced
// plan, 64-feature passes.  The loads of a ragged batch are NOT predicated: the surplus slots re-read the task's last row and are
// selected out.
//   * rows kernel (FORWARD structures, row i owns the task; FWD: NUM and DEN, else dK): the lane group holds K_i (and P_i, O_i) in
//     registers; per entry it reads ONE contiguous 2 f segment [Q_j | V_j] of QV -- a lane its quad of Q and, f floats on, its quad of V
//     -- kRowsInFlight entries (twice as many loads) in flight.
//   * cols kernel (TRANSPOSED structures, row j owns Q_j, V_j): per entry it reads the contiguous 3 f panel row [K_i | P_i | O_i] that
//     the finishing kernel wrote, kColsInFlight entries (three loads each) in flight, and forms dQ_j and dV_j together.
//   * finishing kernel, row-band layout (pgcn_rowband.h): Z1 in place of NUM, or the panel.
// Every product and sum below is an explicit mul / fma on values that no contraction can reach (no product feeds an addition except
// through fmaf), so the float4 body and the scalar body give the same bits.  Inputs are finite by contract.  Plain vector loads and
// stores only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_device.h"
#include "pgcn_internal.h"
#include "pgcn_rowband.h"

namespace {

constexpr int kWavesPerBlock = 4;
static_assert(kThreads == kWavesPerBlock * 64, "the task kernels run 4 waves per block");
constexpr int kRowsInFlight = 8;   // entries per batch of the rows kernel: a quad of Q and of V each = sixteen row loads
constexpr int kColsInFlight = 4;   // entries per batch of the cols kernel: a quad of K, P and O each = twelve row loads
constexpr float kEps = 1e-6f;
constexpr float kClamp = 80.f;

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

// the gate and its complement from one exponential and one reciprocal: e = exp(-x), g = 1 / (1 + e), 1 - g = e g
__device__ __forceinline__ void gate(float k, float q, float &g, float &gc) {
    const float x = fminf(fmaxf(k + q, -kClamp), kClamp);
    const float e = __expf(-x);
    g = __builtin_amdgcn_rcpf(1.f + e);
    gc = e * g;
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
// Over a FORWARD structure.  FWD: OUT = NUM, OUT2 = DEN, OWN = K (ldw).  Otherwise: OUT = dK, OWN = the panel [K | P | O] (planes fp apart).
template <int LPR, int VEC, bool OFF32, bool FWD>
__global__ __launch_bounds__(kThreads, 4) void agggated_rows_kernel(
    const int64_t *__restrict__ rowptr, const uint64_t *__restrict__ pairs, const int4 *__restrict__ tasks, int64_t ntasks,
    const int32_t *__restrict__ slot_row, const float *__restrict__ OWN, int64_t ldw, int32_t fp, const float *__restrict__ QV,
    int64_t ldqv, float *__restrict__ OUT, int64_t ldo, float *__restrict__ OUT2, int64_t ldo2, int32_t f, float *__restrict__ pout,
    float *__restrict__ pout2, int64_t nblocks, uint32_t flags, int32_t nslices, SliceSeg seg) {
    constexpr int U = (LPR < kRowsInFlight) ? LPR : kRowsInFlight;
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

    float kr[VEC], pr[VEC], orow[VEC], a0[VEC], a1[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { kr[v] = 0.f; pr[v] = 0.f; orow[v] = 0.f; a0[v] = 0.f; a1[v] = 0.f; }
    if (tact && fact) {   // this task's own row: K_i (and P_i, O_i)
        const int64_t r = t.dst >= 0 ? slot_row[t.dst] : ~t.dst;
        const float *own = OWN + r * ldw + fcol;
        vload<VEC>(kr, own);
        if constexpr (!FWD) {
            vload<VEC>(pr, own + fp);
            vload<VEC>(orow, own + 2 * fp);
        }
    }

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
            int32_t c[U];
            float q[U][VEC], x[U][VEC];
            if constexpr (U >= 2) {
#pragma unroll
                for (int u = 0; u < U; u += 2) {
                    const int4 w = *reinterpret_cast<const int4 *>(mg + k + u);   // two pairs per LDS read
                    c[u] = w.x;
                    c[u + 1] = w.z;
                }
            } else {
                c[0] = (int32_t)(uint32_t)mg[k];
            }
            if (fact) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float *row = row_at<OFF32>(QV, lane_off, c[u], ldqv);
                    vload<VEC>(q[u], row);
                    vload<VEC>(x[u], row + f);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool ok = k + u < cnt;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        float g, gc;
                        gate(kr[v], q[u][v], g, gc);
                        if constexpr (FWD) {
                            const float n0 = fmaf(g, x[u][v], a0[v]);
                            const float n1 = a1[v] + g;
                            a0[v] = ok ? n0 : a0[v];     // (a select: a surplus slot holds another row's values)
                            a1[v] = ok ? n1 : a1[v];
                        } else {
                            const float pd = pr[v] * (x[u][v] - orow[v]);
                            const float n0 = fmaf(pd, g * gc, a0[v]);
                            a0[v] = ok ? n0 : a0[v];
                        }
                    }
                }
            }
        }
    }

    if (tact && fact) {
        if (t.dst >= 0) {
            vstore<VEC>(pout + (int64_t)t.dst * f + fcol, a0);
            if constexpr (FWD) vstore<VEC>(pout2 + (int64_t)t.dst * f + fcol, a1);
        } else {
            const int64_t row = ~t.dst;
            float *po = OUT + row * ldo + fcol;
            float *po2 = FWD ? OUT2 + row * ldo2 + fcol : nullptr;
            if (flags & PGCN_SPMM_ACCUMULATE) {   // this structure's sums join what the row holds
                float c0[VEC];
                vload<VEC>(c0, po);
#pragma unroll
                for (int v = 0; v < VEC; ++v) a0[v] = c0[v] + a0[v];
                if constexpr (FWD) {
                    vload<VEC>(c0, po2);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) a1[v] = c0[v] + a1[v];
                }
            }
            vstore<VEC>(po, a0);
            if constexpr (FWD) vstore<VEC>(po2, a1);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Over a TRANSPOSED structure: task rows are rows of QV and of D = [dQ | dV], stored entries index the rows of the panel.
template <int LPR, int VEC, bool OFF32>
__global__ __launch_bounds__(kThreads, 4) void agggated_cols_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int4 *__restrict__ tasks, int64_t ntasks,
    const int32_t *__restrict__ slot_row, const float *__restrict__ QV, int64_t ldqv, const float *__restrict__ panel, int64_t ldp,
    int32_t fp, float *__restrict__ D, int64_t ldd, int32_t f, float *__restrict__ pdq, float *__restrict__ pdv, int64_t nblocks,
    uint32_t flags, int32_t nslices, SliceSeg seg) {
    constexpr int U = (LPR < kColsInFlight) ? LPR : kColsInFlight;
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

    float qr[VEC], xr[VEC], dq[VEC], dv[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { qr[v] = 0.f; xr[v] = 0.f; dq[v] = 0.f; dv[v] = 0.f; }
    if (tact && fact) {   // this task's own row [Q_j | V_j]
        const int64_t r = t.dst >= 0 ? slot_row[t.dst] : ~t.dst;
        vload<VEC>(qr, QV + r * ldqv + fcol);
        vload<VEC>(xr, QV + r * ldqv + f + fcol);
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
            float kk[U][VEC], p[U][VEC], o[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) c[u] = mg[k + u];
            if (fact) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float *row = row_at<OFF32>(panel, lane_off, c[u], ldp);
                    vload<VEC>(kk[u], row);
                    vload<VEC>(p[u], row + fp);
                    vload<VEC>(o[u], row + 2 * fp);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool ok = k + u < cnt;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        float g, gc;
                        gate(kk[u][v], qr[v], g, gc);
                        const float pd = p[u][v] * (xr[v] - o[u][v]);
                        const float nq = fmaf(pd, g * gc, dq[v]);
                        const float nv = fmaf(g, p[u][v], dv[v]);
                        dq[v] = ok ? nq : dq[v];     // (a select: a surplus slot holds another row's values)
                        dv[v] = ok ? nv : dv[v];
                    }
                }
            }
        }
    }

    if (tact && fact) {
        if (t.dst >= 0) {
            vstore<VEC>(pdq + (int64_t)t.dst * f + fcol, dq);
            vstore<VEC>(pdv + (int64_t)t.dst * f + fcol, dv);
        } else {
            float *d = D + (int64_t)(~t.dst) * ldd + fcol;
            vstore<VEC>(d, dq);
            vstore<VEC>(d + f, dv);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The finishing kernel, row-band layout.  BWD false: Z = NUM / (DEN + eps) in place of NUM.  BWD true: Z holds Z1 and is read only;
// the panel row [K | P | O] with P = G / (DEN + eps), O = Z1, three planes of fp = 4 ceil(f / 4) words (zeros beyond f).
template <bool VEC, bool BWD>
__global__ __launch_bounds__(kThreads) void agggated_finish_kernel(float *Z, int64_t ldz, const float *__restrict__ DEN, int64_t ldd,
                                                                   int64_t nrows, int f, int log2_tpr, const float *__restrict__ Gm,
                                                                   int64_t ldg, const float *__restrict__ K, int64_t ldk,
                                                                   float *__restrict__ panel, int64_t ldp) {
    const Band b = band_of(log2_tpr, kApplyRows, nrows);
    if (b.c0 >= f) return;
    for (int64_t r = b.r0 + b.rg; r < b.rend; r += b.ngroups) {
        Quad z = load_quad<VEC>(Z + r * ldz, b.c0, f);
        const Quad den = load_quad<VEC>(DEN + r * ldd, b.c0, f);
        if constexpr (!BWD) {
#pragma unroll
            for (int j = 0; j < 4; ++j) z.v[j] = z.v[j] / (den.v[j] + kEps);
            store_quad<VEC>(Z + r * ldz, b.c0, f, z);
        } else {
            Quad p = load_quad<VEC>(Gm + r * ldg, b.c0, f);
#pragma unroll
            for (int j = 0; j < 4; ++j) p.v[j] = p.v[j] / (den.v[j] + kEps);
            const int fp = (f + 3) & ~3;                               // (the planes are whole quads: float4 stores, zeros beyond f)
            float *row = panel + r * ldp + b.c0;
            store_quad<true>(row, 0, fp, load_quad<VEC>(K + r * ldk, b.c0, f));
            store_quad<true>(row, fp, 2 * fp, p);
            store_quad<true>(row, 2 * fp, 3 * fp, z);
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

// a structure and its plan as the entry points take them
struct Plan {
    const int64_t *rowptr;
    const int32_t *ent;          // pairs (forward structures) or col (transposed)
    const int32_t *slot_row, *tasks;
    int64_t ntasks;
    const int64_t *seg;
    int32_t nslices;
    const int32_t *fix;
    int64_t nfix, nslots;
};

// the checks every task entry point makes before any launch; 1: nothing to do
int check_plan(const Plan &p, int32_t f, const char *who) {
    if (p.ntasks < 0 || p.nfix < 0 || p.nslots < 0 || f < 1 || p.nslices < 1 || p.nslices > PGCN_MAX_SLICES ||
        (p.nslices > 1 && (!p.seg || !p.tasks)))
        return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes");
    if (p.nslices > 1 && (p.seg[0] != 0 || p.seg[p.nslices] != p.ntasks))
        return pgcn_set_error2(PGCN_EINVAL, who, "seg does not cover the task list");
    if (p.ntasks == 0) return 1;
    if (!p.rowptr || !p.ent || (p.nfix > 0 && (!p.fix || !p.tasks)) || (p.nslots > 0 && !p.slot_row))
        return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    if (p.ntasks > 0x7fffffffLL) return pgcn_set_error2(PGCN_EINVAL, who, "ntasks >= 2^31");
    return PGCN_OK;
}

// PGCN_SPMM_OFFSETS32 promises that the byte offset of every row of the gathered operand (ncols rows, ld floats apart) fits 32 bits
bool offsets32_bad(uint32_t flags, int64_t ncols, int64_t ld) {
    return (flags & PGCN_SPMM_OFFSETS32) && (ncols < 0 || ld > 0x3fffffffLL || ncols * ld * 4 > 0xffffffffLL);
}

bool al16(const void *p) { return (uintptr_t)p % 16 == 0; }

template <int LPR, int VEC, bool FWD>
int launch_rows(const Plan &p, const float *OWN, int64_t ldw, int32_t fp, const float *QV, int64_t ldqv, float *OUT, int64_t ldo,
                float *OUT2, int64_t ldo2, int32_t f, float *pout, float *pout2, uint32_t flags, hipStream_t s, const char *who) {
    SliceSeg seg{};
    const Grid g = task_grid<LPR, VEC>(p.ntasks, f, flags, p.nslices, p.seg, seg);
    if (g.blocks > 0x7fffffffLL) return pgcn_set_error2(PGCN_EINVAL, who, "too many tasks for one launch");
    const uint64_t *p64 = reinterpret_cast<const uint64_t *>(p.ent);
    const int4 *t4 = reinterpret_cast<const int4 *>(p.tasks);
    if (flags & PGCN_SPMM_OFFSETS32)
        hipLaunchKernelGGL((agggated_rows_kernel<LPR, VEC, true, FWD>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s, p.rowptr,
                           p64, t4, p.ntasks, p.slot_row, OWN, ldw, fp, QV, ldqv, OUT, ldo, OUT2, ldo2, f, pout, pout2, g.blocks, flags,
                           p.nslices, seg);
    else
        hipLaunchKernelGGL((agggated_rows_kernel<LPR, VEC, false, FWD>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s, p.rowptr,
                           p64, t4, p.ntasks, p.slot_row, OWN, ldw, fp, QV, ldqv, OUT, ldo, OUT2, ldo2, f, pout, pout2, g.blocks, flags,
                           p.nslices, seg);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

template <int LPR, int VEC>
int launch_cols(const Plan &p, const float *QV, int64_t ldqv, const float *panel, int64_t ldp, int32_t fp, float *D, int64_t ldd,
                int32_t f, float *pdq, float *pdv, uint32_t flags, hipStream_t s, const char *who) {
    SliceSeg seg{};
    const Grid g = task_grid<LPR, VEC>(p.ntasks, f, flags, p.nslices, p.seg, seg);
    if (g.blocks > 0x7fffffffLL) return pgcn_set_error2(PGCN_EINVAL, who, "too many tasks for one launch");
    const int4 *t4 = reinterpret_cast<const int4 *>(p.tasks);
    if (flags & PGCN_SPMM_OFFSETS32)
        hipLaunchKernelGGL((agggated_cols_kernel<LPR, VEC, true>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s, p.rowptr, p.ent,
                           t4, p.ntasks, p.slot_row, QV, ldqv, panel, ldp, fp, D, ldd, f, pdq, pdv, g.blocks, flags, p.nslices, seg);
    else
        hipLaunchKernelGGL((agggated_cols_kernel<LPR, VEC, false>), dim3((unsigned)g.blocks, g.ntiles), dim3(kThreads), 0, s, p.rowptr, p.ent,
                           t4, p.ntasks, p.slot_row, QV, ldqv, panel, ldp, fp, D, ldd, f, pdq, pdv, g.blocks, flags, p.nslices, seg);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

}  // namespace

#define PGCN_AGGGATED_SHAPES(CASE)                                                         \
    CASE(1, 4) CASE(2, 4) CASE(4, 4) CASE(8, 4) CASE(16, 4) CASE(32, 4) CASE(64, 4)        \
    CASE(1, 1) CASE(2, 1) CASE(4, 1) CASE(8, 1) CASE(16, 1) CASE(32, 1) CASE(64, 1)

extern "C" int pgcn_agggated_csr_plan_f32(const int64_t *rowptr, const int32_t *pairs, const int32_t *slot_row, const int32_t *tasks,
                                          int64_t ntasks, const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix,
                                          int64_t ncols, const float *K, int64_t ldk, const float *QV, int64_t ldqv, float *NUM, int64_t ldn, float *DEN,
                                          int64_t ldd, int32_t f, void *ws, int64_t ws_bytes, int64_t nslots, uint32_t flags,
                                          pgcn_stream_t stream) {
    static const char *who = "pgcn_agggated_csr_plan_f32";
    const Plan p{rowptr, pairs, slot_row, tasks, ntasks, seg, nslices, fix, nfix, nslots};
    if (int rc = check_plan(p, f, who)) return rc == 1 ? PGCN_OK : rc;
    if (ldk < f || ldqv < 2 * (int64_t)f || ldn < f || ldd < f) return pgcn_set_error2(PGCN_EINVAL, who, "a leading dimension is too small");
    if (!K || !QV || !NUM || !DEN || (nslots > 0 && !ws)) return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    if ((uintptr_t)pairs % 8 != 0) return pgcn_set_error2(PGCN_EINVAL, who, "pairs must be 8-byte aligned");
    if (offsets32_bad(flags, ncols, ldqv)) return pgcn_set_error2(PGCN_EINVAL, who, "offsets beyond 32 bits under PGCN_SPMM_OFFSETS32");
    if (ws_bytes < nslots * (int64_t)f * 8) return pgcn_set_error2(PGCN_ENOMEM, who, "work-space too small");
    float *pnum = reinterpret_cast<float *>(ws);                 // NUM plane, then DEN plane: nslots x f each
    float *pden = reinterpret_cast<float *>(ws) + nslots * (int64_t)f;
    const Shape sh = pick_shape(f, f % 4 == 0 && al16(K) && al16(QV) && al16(NUM) && al16(DEN) && al16(pnum) && al16(pden) && ldk % 4 == 0 &&
                                       ldqv % 4 == 0 && ldn % 4 == 0 && ldd % 4 == 0, flags);
    int rc = 1;   // (no shape taken yet)
#define PGCN_CASE(L, V)                                                                                                              \
    if (sh.lpr == L && sh.vec == V)                                                                                                  \
        rc = launch_rows<L, V, true>(p, K, ldk, 0, QV, ldqv, NUM, ldn, DEN, ldd, f, pnum, pden, flags, (hipStream_t)stream, who);
    PGCN_AGGGATED_SHAPES(PGCN_CASE)
#undef PGCN_CASE
    if (rc == 1) return pgcn_set_error2(PGCN_EINVAL, who, "no kernel shape");
    if (rc != PGCN_OK || nfix == 0) return rc;
    // the pieces of a cut row, added in slot order (the sum path's fix-up: the slots hold plain partial sums)
    rc = pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, pnum, NUM, ldn, f, flags & PGCN_SPMM_ACCUMULATE, stream);
    if (rc != PGCN_OK) return rc;
    return pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, pden, DEN, ldd, f, flags & PGCN_SPMM_ACCUMULATE, stream);
}

extern "C" int pgcn_agggated_finish_f32(float *Z, int64_t ldz, const float *DEN, int64_t ldd, int64_t nrows, int32_t f, const float *G,
                                        int64_t ldg, const float *K, int64_t ldk, float *panel, int64_t ldp, pgcn_stream_t stream) {
    static const char *who = "pgcn_agggated_finish_f32";
    const bool bwd = G != nullptr;
    if (nrows < 0 || f < 1 || f > kMaxF) return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes (1 <= f <= 1024)");
    if (ldz < f || ldd < f || (bwd && (ldg < f || ldk < f || ldp < 3 * (((int64_t)f + 3) & ~3LL))))
        return pgcn_set_error2(PGCN_EINVAL, who, "a leading dimension is too small (ldp >= 12 ceil(f / 4))");
    if (nrows == 0) return PGCN_OK;
    if (!Z || !DEN || (bwd && (!K || !panel))) return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    if (bwd && (!aligned16(panel) || !rows16(ldp))) return pgcn_set_error2(PGCN_EINVAL, who, "the panel and its rows must be 16-byte aligned");
    const int64_t nblocks = apply_blocks(nrows);
    if (nblocks > 0x7fffffffLL) return pgcn_set_error2(PGCN_EINVAL, who, "too many rows");
    const int l2 = log2_threads_per_row(f);
    const bool vec = f % 4 == 0 && rows16(ldz) && rows16(ldd) && aligned16(Z) && aligned16(DEN) &&
                     (!bwd || (rows16(ldg) && rows16(ldk) && aligned16(G) && aligned16(K)));
    hipStream_t s = (hipStream_t)stream;
    if (bwd)
        launch(vec ? agggated_finish_kernel<true, true> : agggated_finish_kernel<false, true>, nblocks, s, Z, ldz, DEN, ldd, nrows, f, l2, G,
               ldg, K, ldk, panel, ldp);
    else
        launch(vec ? agggated_finish_kernel<true, false> : agggated_finish_kernel<false, false>, nblocks, s, Z, ldz, DEN, ldd, nrows, f, l2, G,
               ldg, K, ldk, panel, ldp);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_agggated_grad_rows_f32(const int64_t *rowptr, const int32_t *pairs, const int32_t *slot_row, const int32_t *tasks,
                                           int64_t ntasks, const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix,
                                           int64_t ncols, const float *panel, int64_t ldp, const float *QV, int64_t ldqv, float *dK, int64_t lddk,
                                           int32_t f, float *partial_ws, int64_t partial_ws_elems, int64_t nslots, uint32_t flags,
                                           pgcn_stream_t stream) {
    static const char *who = "pgcn_agggated_grad_rows_f32";
    const Plan p{rowptr, pairs, slot_row, tasks, ntasks, seg, nslices, fix, nfix, nslots};
    if (int rc = check_plan(p, f, who)) return rc == 1 ? PGCN_OK : rc;
    const int32_t fp = (f + 3) & ~3;
    if (ldp < 3 * (int64_t)fp || ldqv < 2 * (int64_t)f || lddk < f) return pgcn_set_error2(PGCN_EINVAL, who, "a leading dimension is too small");
    if (!panel || !QV || !dK || (nslots > 0 && !partial_ws)) return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    if ((uintptr_t)pairs % 8 != 0) return pgcn_set_error2(PGCN_EINVAL, who, "pairs must be 8-byte aligned");
    if (offsets32_bad(flags, ncols, ldqv)) return pgcn_set_error2(PGCN_EINVAL, who, "offsets beyond 32 bits under PGCN_SPMM_OFFSETS32");
    if (partial_ws_elems < nslots * (int64_t)f) return pgcn_set_error2(PGCN_ENOMEM, who, "partial work-space too small");
    const Shape sh = pick_shape(f, f % 4 == 0 && al16(panel) && al16(QV) && al16(dK) && al16(partial_ws) && ldp % 4 == 0 && ldqv % 4 == 0 &&
                                       lddk % 4 == 0, flags);
    int rc = 1;
#define PGCN_CASE(L, V)                                                                                                              \
    if (sh.lpr == L && sh.vec == V)                                                                                                  \
        rc = launch_rows<L, V, false>(p, panel, ldp, fp, QV, ldqv, dK, lddk, nullptr, 0, f, partial_ws, nullptr, flags,             \
                                      (hipStream_t)stream, who);
    PGCN_AGGGATED_SHAPES(PGCN_CASE)
#undef PGCN_CASE
    if (rc == 1) return pgcn_set_error2(PGCN_EINVAL, who, "no kernel shape");
    if (rc != PGCN_OK || nfix == 0) return rc;
    return pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_ws, dK, lddk, f, flags & PGCN_SPMM_ACCUMULATE, stream);
}

extern "C" int pgcn_agggated_grad_cols_f32(const int64_t *rowptr, const int32_t *col, const int32_t *slot_row, const int32_t *tasks,
                                           int64_t ntasks, const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix,
                                           int64_t ncols, const float *QV, int64_t ldqv, const float *panel, int64_t ldp, float *D, int64_t ldd, int32_t f,
                                           void *ws, int64_t ws_bytes, int64_t nslots, uint32_t flags, pgcn_stream_t stream) {
    static const char *who = "pgcn_agggated_grad_cols_f32";
    const Plan p{rowptr, col, slot_row, tasks, ntasks, seg, nslices, fix, nfix, nslots};
    if (int rc = check_plan(p, f, who)) return rc == 1 ? PGCN_OK : rc;
    const int32_t fp = (f + 3) & ~3;
    if (ldqv < 2 * (int64_t)f || ldp < 3 * (int64_t)fp || ldd < 2 * (int64_t)f)
        return pgcn_set_error2(PGCN_EINVAL, who, "a leading dimension is too small");
    if (!QV || !panel || !D || (nslots > 0 && !ws)) return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    if (offsets32_bad(flags, ncols, ldp)) return pgcn_set_error2(PGCN_EINVAL, who, "offsets beyond 32 bits under PGCN_SPMM_OFFSETS32");
    if (ws_bytes < nslots * (int64_t)f * 8) return pgcn_set_error2(PGCN_ENOMEM, who, "work-space too small");
    float *pdq = reinterpret_cast<float *>(ws);                  // dQ plane, then dV plane: nslots x f each
    float *pdv = reinterpret_cast<float *>(ws) + nslots * (int64_t)f;
    const Shape sh = pick_shape(f, f % 4 == 0 && al16(QV) && al16(panel) && al16(D) && al16(pdq) && al16(pdv) && ldqv % 4 == 0 && ldp % 4 == 0 &&
                                       ldd % 4 == 0, flags);
    int rc = 1;
#define PGCN_CASE(L, V)                                                                                                              \
    if (sh.lpr == L && sh.vec == V)                                                                                                  \
        rc = launch_cols<L, V>(p, QV, ldqv, panel, ldp, fp, D, ldd, f, pdq, pdv, flags, (hipStream_t)stream, who);
    PGCN_AGGGATED_SHAPES(PGCN_CASE)
#undef PGCN_CASE
    if (rc == 1) return pgcn_set_error2(PGCN_EINVAL, who, "no kernel shape");
    if (rc != PGCN_OK || nfix == 0) return rc;
    // the pieces of a cut row, added in slot order: D is written, whatever it held
    rc = pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, pdq, D, ldd, f, 0u, stream);
    if (rc != PGCN_OK) return rc;
    return pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, pdv, D + f, ldd, f, 0u, stream);
}
