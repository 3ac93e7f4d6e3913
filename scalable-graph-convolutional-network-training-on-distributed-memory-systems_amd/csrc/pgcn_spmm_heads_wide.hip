// pgcn_spmm_heads_wide.hip -- the two recomputing gather passes of the v1 attention layer for rows of 257 to 1024
// columns (gfx950), fp32: 8 x 64, 4 x 128 (512 columns), 4 x 256, 8 x 128 (1024), everything between with d = 64, 128, 256.
//
// The kernels of pgcn_spmm_heads.hip give a lane four features, so a wave covers 256 columns and no more.  Two passes over
// head groups of 256 columns are not the answer: what a pass pays PER ENTRY -- the column id, the row statistics, `heads`
// exponentials, the parked words, the reduction -- is most of its cost (profiles/r04_gat_head_groups.txt: half the panel
// costs 74 % of the whole pass).  Here ONE wave still owns a task of the plan and pays all of that once per entry, for a
// row that is R = ceil(F / 256) WINDOWS wide:
//   * a lane owns R float4 segments, at columns 256 r + 4 lane.  d divides 256, so no head straddles a window and the
//     lanes of a head are the same d / 4 lanes in every window: head of (window r, lane l) = (256 r + 4 l) / d;
//   * col and the `heads` weights (FWD: and c values; GRAD: A and t) of 64 entries are computed lane-parallel -- one lane,
//     one entry, all heads -- and parked in the wave's private LDS; the gather loop reads col as a broadcast and one word
//     per window (FWD: two);
//   * gathers go out unpredicated, NB entries x R windows of 16 bytes per lane at a time: NB = 8 at R = 2, 4 at R = 3 and
//     4, which keeps the rows in flight at <= 64 registers and the kernel out of scratch.  A ragged batch re-reads the
//     task's last referenced row and selects it away: nothing the task does not reference is ever combined;
//   * GRAD: the NB x R dot products <dOut_i, Z_j> per head of a batch are 16 values per lane (R = 3: four of them zero),
//     summed over the 16 lanes of a DPP row by ONE transposing reduction -- every step halves the values a lane carries
//     while it doubles the lanes summed, 15 DPP moves for 16 sums -- and over the 2 or 4 rows of a wider head by one or
//     two cross-row exchanges.  Lane l of a row finishes value l = (entry l / RP, window l % RP): a fixed window, so its
//     running sum of de belongs to ONE head, and ds2 is a reduction over the lanes of equal window at the end of the task;
//   * cut rows leave partial rows in slots, combined in slot order by pgcn_spmm_fixup_f32.  No atomics; the order of
//     every sum is fixed by the plan: two runs give the same bits.
// The arithmetic per entry and its order along a row are those of the narrow kernels; the per-entry gradient is never
// stored (de of pgcn_spmm_heads_grad_f32 has no counterpart here).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pgcn_device.h"
#include "pgcn_internal.h"
#include "pgcn_spmm_heads.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kMaxHeads = 8;
constexpr int kWindow = 256;               // columns a wave covers with one float4 per lane
constexpr int kMaxWindows = 4;

template <int KH, int R, bool GRAD>
__global__ __launch_bounds__(kThreads, 2) void spmm_heads_wide_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int4 *__restrict__ tasks, int64_t ntasks,
    const float *__restrict__ B, int64_t ldb, float *__restrict__ C, int64_t ldc, int32_t F, int32_t d,
    float *__restrict__ partial, uint32_t flags, int32_t nslices, SliceSeg seg, Recompute rc, EdgeGrad eg, Forward2 f2) {
    constexpr bool FWD = !GRAD;
    constexpr int PS = GRAD ? 3 * KH + 1 : 2 * KH + 1;      // parked words per entry: col, alpha[KH], then c[KH] | A[KH], t[KH]
    constexpr int RP = R == 2 ? 2 : 4;                      // R rounded up to a power of two
    constexpr int NB = 16 / RP;                             // entries per gather batch
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
    const int dsh = __ffs(d) - 1;              // d = 64, 128 or 256
    const int hl = d >> 2;                     // lanes per head: 16, 32 or 64
    int fcol[R], fsafe[R], head[R];
    bool fact[R];                              // (only the last window can be partly empty; its idle lanes are whole heads)
#pragma unroll
    for (int r = 0; r < R; ++r) {
        fcol[r] = r * kWindow + lane * 4;
        fact[r] = fcol[r] < F;
        fsafe[r] = fact[r] ? fcol[r] : 0;
        head[r] = fact[r] ? fcol[r] >> dsh : 0;
    }
    f32x2 accl[R], acch[R];                    // this lane's four features per window of the output row
    f32x2 sl[R], sh[R];                        // FWD: ... and of V;  GRAD: this lane's features of Z_j
    float csum[KH];                            // FWD: this lane's share of C_i
#pragma unroll
    for (int r = 0; r < R; ++r) accl[r] = acch[r] = sl[r] = sh[r] = f32x2{0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KH; ++k) csum[k] = 0.f;
    float *mine = park[wave];
    const int last = len > 0 ? len - 1 : 0;
    int64_t row = 0;
    if (len > 0) {
        if (dst < 0) {
            row = ~dst;
        } else {                               // largest row with rowptr[row] <= kbeg (a split row is never empty)
            int64_t lo = 0, hi = rc.nrows - 1;
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (rowptr[mid] <= kbeg) lo = mid; else hi = mid - 1;
            }
            row = lo;
        }
    }
    float a2[KH];                              // GRAD: s2 of this task's row
#pragma unroll
    for (int k = 0; k < KH; ++k) a2[k] = 0.f;
    // GRAD: the value of the batch's 16 this lane finishes -- entry u_m of the batch, window r_m -- and whether it is the
    // one lane of its head that does (the first DPP row of the head's lanes, a window that exists, a head that exists)
    const int u_m = (lane & 15) / RP, r_m = (lane & 15) % RP;
    const int fcol_m = r_m * kWindow + lane * 4;
    const bool writer = (lane & (hl - 1)) < 16 && r_m < R && fcol_m < F;
    const int head_m = writer ? fcol_m >> dsh : 0;
    float acc2 = 0.f;
    if constexpr (GRAD) {
        if (len > 0) {
#pragma unroll
            for (int k = 0; k < KH; ++k) a2[k] = rc.s2[row * rc.lds2 + k];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (fact[r]) {
                    float zr[4];
                    vload<4>(zr, eg.Z + row * eg.ldz + fcol[r]);
                    sl[r] = f32x2{zr[0], zr[1]};
                    sh[r] = f32x2{zr[2], zr[3]};
                }
            }
        }
    }
    // the KH weights of the entry with column c -- the arithmetic of pgcn_spmm_heads.hip.  FWD: from the statistics of the
    // task's row and s2 of c, ga = c_ij;  GRAD: from the statistics of row c and s2 of the task's row, ga = (alpha + beta)
    // [x LeakyReLU'], gt = t of row c
    auto weights = [&](int32_t c, float (&w)[KH], float (&ga)[KH], float (&gt)[KH]) {
        float4 q[KH];
        float sv[KH];
        if constexpr (FWD) {
#pragma unroll
            for (int k = 0; k < KH; ++k) q[k] = rc.rowstat[row * KH + k];      // (one line, the same for all lanes)
#pragma unroll
            for (int k = 0; k < KH; ++k) sv[k] = rc.s2[(int64_t)c * rc.lds2 + k];
        } else {
#pragma unroll
            for (int k = 0; k < KH; ++k) q[k] = rc.rowstat[(int64_t)c * KH + k];
#pragma unroll
            for (int k = 0; k < KH; ++k) {
                sv[k] = a2[k];
                gt[k] = eg.t[(int64_t)c * KH + k];
            }
        }
#pragma unroll
        for (int k = 0; k < KH; ++k) {
            const float raw = q[k].x + sv[k];
            float r = raw;
            if (rc.mode == 0) r = r > 0.f ? r : r * rc.slope;
            w[k] = (expf(r - q[k].y) - q[k].w) * q[k].z;
            if constexpr (FWD) {
                ga[k] = rc.mode == 0 ? w[k] * (raw > 0.f ? 1.f : rc.slope) : w[k] + q[k].w * q[k].z;
            } else {
                float g = w[k] + (rc.mode == 1 ? q[k].w * q[k].z : 0.f);
                if (rc.mode == 0) g *= raw > 0.f ? 1.f : rc.slope;
                ga[k] = g;
            }
        }
    };
    // prefetch of the first 64 tuples: unconditional, index clamped into the task
    int32_t nc = 0;
    float na[KH], nga[KH], ngt[KH];
#pragma unroll
    for (int k = 0; k < KH; ++k) na[k] = nga[k] = ngt[k] = 0.f;
    if (len > 0) {
        const int e = lane < last ? lane : last;
        nc = __builtin_nontemporal_load(col + kbeg + e);
        weights(nc, na, nga, ngt);
        if constexpr (FWD) {
#pragma unroll
            for (int k = 0; k < KH; ++k) csum[k] += lane < len ? nga[k] : 0.f;
        }
    }
    for (int base = 0; base < len; base += 64) {   // wave-uniform: one task per wave
        __builtin_amdgcn_wave_barrier();
        mine[lane * PS] = __int_as_float(nc);
#pragma unroll
        for (int k = 0; k < KH; ++k) {
            mine[lane * PS + 1 + k] = na[k];
            mine[lane * PS + 1 + KH + k] = nga[k];
            if constexpr (GRAD) mine[lane * PS + 1 + 2 * KH + k] = ngt[k];
        }
        __builtin_amdgcn_wave_barrier();
        if (base + 64 < len) {
            int e = base + 64 + lane;
            e = e < last ? e : last;
            nc = __builtin_nontemporal_load(col + kbeg + e);
            weights(nc, na, nga, ngt);
            if constexpr (FWD) {
#pragma unroll
                for (int k = 0; k < KH; ++k) csum[k] += base + 64 + lane < len ? nga[k] : 0.f;
            }
        }
        const int cnt = min(64, len - base);
        for (int e0 = 0; e0 < cnt; e0 += NB) {
            int32_t c[NB];
            float x[NB][R][4];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int e = e0 + u < cnt ? e0 + u : cnt - 1;       // ragged tail: the task's last referenced row
                c[u] = __float_as_int(mine[e * PS]);
            }
            // (lanes beyond the F features gather column 0 and are never stored: no branch around the gathers)
#pragma unroll
            for (int u = 0; u < NB; ++u) {
#pragma unroll
                for (int r = 0; r < R; ++r) vload<4>(x[u][r], B + (int64_t)c[u] * ldb + fsafe[r]);
            }
            float dq[16];                      // GRAD: dq[u * RP + r] = this lane's part of <dOut_i, Z_j> in window r
#pragma unroll
            for (int v = 0; v < 16; ++v) dq[v] = 0.f;
            // full batches (all but a task's last) take packed FMAs and no selects
            auto combine = [&](auto full) {
                constexpr bool FULL = decltype(full)::value;
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const bool keep = FULL || e0 + u < cnt;
                    const int e = keep ? e0 + u : cnt - 1;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const float w = keep ? mine[e * PS + 1 + head[r]] : 0.f;
                        const f32x2 ww = {w, w};
                        const f32x2 xl = {keep ? x[u][r][0] : 0.f, keep ? x[u][r][1] : 0.f};
                        const f32x2 xh = {keep ? x[u][r][2] : 0.f, keep ? x[u][r][3] : 0.f};
                        accl[r] = __builtin_elementwise_fma(ww, xl, accl[r]);
                        acch[r] = __builtin_elementwise_fma(ww, xh, acch[r]);
                        if constexpr (FWD) {
                            const float w2 = keep ? mine[e * PS + 1 + KH + head[r]] : 0.f;
                            const f32x2 w22 = {w2, w2};
                            sl[r] = __builtin_elementwise_fma(w22, xl, sl[r]);
                            sh[r] = __builtin_elementwise_fma(w22, xh, sh[r]);
                        } else {
                            const f32x2 pr = __builtin_elementwise_fma(xh, sh[r], xl * sl[r]);
                            dq[u * RP + r] = pr.x + pr.y;
                        }
                    }
                }
            };
            if (e0 + NB <= cnt) combine(std::true_type{}); else combine(std::false_type{});
            if constexpr (GRAD) {
                // 16 values x 16 lanes: the transposing reduction on the DPP network.  Lane l of a row ends with value l
                const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2, b0 = lane & 1;
                float r1[8], r2[4], r3[2];
#pragma unroll
                for (int v = 0; v < 8; ++v)
                    r1[v] = (b3 ? dq[v + 8] : dq[v]) + dpp_f<0x128>(b3 ? dq[v] : dq[v + 8]);          // row_ror:8 = lane ^ 8
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    r2[v] = (b2 ? r1[v + 4] : r1[v]) + dpp_xor4(b2 ? r1[v] : r1[v + 4]);
#pragma unroll
                for (int v = 0; v < 2; ++v)
                    r3[v] = (b1 ? r2[v + 2] : r2[v]) + dpp_f<0x4E>(b1 ? r2[v] : r2[v + 2]);           // quad_perm [2,3,0,1]
                float dm = (b0 ? r3[1] : r3[0]) + dpp_f<0xB1>(b0 ? r3[0] : r3[1]);                   // quad_perm [1,0,3,2]
                if (hl >= 32) dm += __shfl_xor(dm, 16, 64);      // (wave-uniform: the other rows of a wider head)
                if (hl == 64) dm += __shfl_xor(dm, 32, 64);
                const int e = e0 + u_m;
                if (writer && e < cnt)
                    acc2 += mine[e * PS + 1 + KH + head_m] * (dm - mine[e * PS + 1 + 2 * KH + head_m]);
            }
        }
    }
    const int64_t pw = GRAD ? (int64_t)eg.pw : (int64_t)F;     // width of a partial row
    if constexpr (GRAD) {
        // ds2 of the row = the task's sum of de per head.  A lane's sum belongs to head (window r_m, lane group): add the
        // lanes of equal window -- the bits above RP of the lane's place in its row, then the rows of a wider head (which
        // hold zero) -- and lane L < pw - F writes column F + L, taken from the first lane of head L's group with window
        // L / (heads per window) (pad columns: zero)
        for (int o = RP; o < 16; o <<= 1) acc2 += __shfl_xor(acc2, o, 64);
        for (int o = 16; o < hl; o <<= 1) acc2 += __shfl_xor(acc2, o, 64);
        const int hw = kWindow >> dsh;         // heads per window
        const int k = lane < KH ? lane : KH - 1;
        const float v = __shfl(acc2, (k % hw) * hl + k / hw, 64);
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
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (fact[r]) {
                    float v4[4] = {sl[r].x, sl[r].y, sh[r].x, sh[r].y};
                    if (add) {
                        float old[4];
                        vload<4>(old, o2 + fcol[r]);
#pragma unroll
                        for (int v = 0; v < 4; ++v) v4[v] += old[v];
                    }
                    vstore<4>(o2 + fcol[r], v4);
                }
            }
            if (lane < f2.pw2 - F) {
                float out = lane < KH ? mysum : 0.f;
                if (add) out += o2[F + lane];
                o2[F + lane] = out;
            }
        }
    }
    if (tact) {
        float *o = dst >= 0 ? partial + (int64_t)dst * pw : C + (int64_t)(~dst) * ldc;
        const bool add = dst < 0 && (flags & PGCN_SPMM_ACCUMULATE);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (fact[r]) {
                float acc[4] = {accl[r].x, accl[r].y, acch[r].x, acch[r].y};
                if (add) {
                    float old[4];
                    vload<4>(old, o + fcol[r]);
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[v] += old[v];
                }
                vstore<4>(o + fcol[r], acc);
            }
        }
    }
}

// Validation of both entry points (nothing is launched before all of it has passed), the grid of the sliced plan, the
// launch and the fix-up of cut rows.  eg != NULL: the backward pass; otherwise f2 != NULL: the forward pass.
int launch_wide(const char *who, const int64_t *rowptr, const int32_t *col, const Recompute &rc, const EdgeGrad *eg,
                const Forward2 *f2, int32_t heads, int32_t d, int64_t nrows, const int32_t *tasks, int64_t ntasks,
                const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const float *B, int64_t ldb, float *C,
                int64_t ldc, float *partial_ws, int64_t partial_ws_elems, int64_t nslots, uint32_t flags, pgcn_stream_t stream) {
    const int64_t F = (int64_t)heads * d;
    if (heads <= 0 || d <= 0 || nrows < 0 || ntasks < 0 || nfix < 0 || nslots < 0 || nslices < 1 || nslices > PGCN_MAX_SLICES ||
        ldb < F || ldc < F || (nslices > 1 && (!seg || !tasks)))
        return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes");
    if (heads > kMaxHeads || (d != 64 && d != 128 && d != 256) || F <= kWindow || F > kMaxWindows * kWindow)
        return pgcn_set_error2(PGCN_EUNSUPPORTED, who, "needs heads <= 8, d = 64, 128 or 256 and 256 < heads * d <= 1024 "
                                                       "(narrower rows: pgcn_spmm_heads_*_f32)");
    if (eg && eg->de)
        return pgcn_set_error2(PGCN_EUNSUPPORTED, who, "the per-entry gradient is not kept at these widths: de must be NULL");
    if (ldb % 4 || ldc % 4 || (uintptr_t)B % 16 || (uintptr_t)C % 16 || (uintptr_t)partial_ws % 16)
        return pgcn_set_error2(PGCN_EUNSUPPORTED, who, "needs 16-byte aligned operands and leading dimensions that are multiples of 4");
    const int64_t nt = tasks ? ntasks : nrows;
    if (nt == 0) return PGCN_OK;
    if (!rowptr || !col || !B || !C || (nfix > 0 && !fix) || (nslots > 0 && !partial_ws))
        return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    if (!rc.rowstat || !rc.s2 || rc.lds2 < heads || (uintptr_t)rc.rowstat % 16 || (rc.mode != 0 && rc.mode != 1))
        return pgcn_set_error2(PGCN_EINVAL, who, "bad row statistics / s2 / mode");
    const int64_t pwx = F + (heads + 3) / 4 * 4;         // an output row with the per-head columns behind the features
    int64_t pw_all;                                      // floats of work-space per slot
    Forward2 h0{};
    if (eg) {
        if (!eg->Z || !eg->t || eg->ldz < F || eg->ldz % 4 || (uintptr_t)eg->Z % 16)
            return pgcn_set_error2(PGCN_EINVAL, who, "bad Z / t");
        if (ldc < pwx)
            return pgcn_set_error2(PGCN_EINVAL, who, "C must hold heads * d + heads (rounded up to 4) columns");
        pw_all = pwx;
    } else {
        if (!f2->C2 || f2->ldc2 < pwx || f2->ldc2 % 4 || (uintptr_t)f2->C2 % 16)
            return pgcn_set_error2(PGCN_EINVAL, who, "bad second output (heads * d + heads columns, rounded up to 4)");
        pw_all = F + pwx;
        h0 = *f2;
        h0.partial2 = partial_ws ? partial_ws + nslots * F : nullptr;
    }
    if (partial_ws_elems < nslots * pw_all)
        return pgcn_set_error2(PGCN_ENOMEM, who, "partial work-space too small");
    SliceSeg sg{};
    int64_t grid;
    if (nslices > 1) {
        if (seg[0] != 0 || seg[nslices] != ntasks)
            return pgcn_set_error2(PGCN_EINVAL, who, "seg does not cover the task list");
        int64_t longest = 0;
        for (int i = 0; i <= nslices; ++i) sg.v[i] = seg[i];
        for (int i = 0; i < nslices; ++i) longest = sg.v[i + 1] - sg.v[i] > longest ? sg.v[i + 1] - sg.v[i] : longest;
        grid = ((longest + kWaves - 1) / kWaves) * nslices;
    } else {
        grid = (nt + kWaves - 1) / kWaves;
    }
    if (grid > 0x7fffffffLL) return pgcn_set_error2(PGCN_EINVAL, who, "too many tasks for one launch");
    hipStream_t s = (hipStream_t)stream;
    const int4 *t4 = reinterpret_cast<const int4 *>(tasks);
    EdgeGrad g0{};
    if (eg) g0 = *eg;
    const int R = (int)((F + kWindow - 1) / kWindow);
#define PGCN_WIDE_LAUNCH(KH, R, GR)                                                                                       \
    hipLaunchKernelGGL((spmm_heads_wide_kernel<KH, R, GR>), dim3((unsigned)grid), dim3(kThreads), 0, s, rowptr, col, t4, \
                       nt, B, ldb, C, ldc, (int32_t)F, d, partial_ws, flags, nslices, sg, rc, g0, h0)
#define PGCN_WIDE(KH, R)                                                                                                 \
    case KH * 8 + R:                                                                                                     \
        if (eg) PGCN_WIDE_LAUNCH(KH, R, true);                                                                           \
        else PGCN_WIDE_LAUNCH(KH, R, false);                                                                             \
        break;
    switch (heads * 8 + R) {       // every (heads, windows) of d = 64 (5..8 heads), 128 (3..8) and 256 (2..4)
        PGCN_WIDE(2, 2) PGCN_WIDE(3, 2) PGCN_WIDE(3, 3) PGCN_WIDE(4, 2) PGCN_WIDE(4, 4) PGCN_WIDE(5, 2) PGCN_WIDE(5, 3)
        PGCN_WIDE(6, 2) PGCN_WIDE(6, 3) PGCN_WIDE(7, 2) PGCN_WIDE(7, 4) PGCN_WIDE(8, 2) PGCN_WIDE(8, 4)
        default: return pgcn_set_error2(PGCN_EUNSUPPORTED, who, "no kernel for this (heads, d)");
    }
#undef PGCN_WIDE
#undef PGCN_WIDE_LAUNCH
    PGCN_HIP_CHECK(hipGetLastError());
    if (nfix > 0) {    // (GRAD: the ds2 columns of a cut row are combined with its features, one list, one launch)
        const int rcf = pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, partial_ws, C, ldc, (int32_t)(eg ? pwx : F),
                                            flags & PGCN_SPMM_ACCUMULATE, stream);
        if (rcf != PGCN_OK || eg) return rcf;
        return pgcn_spmm_fixup_f32(fix, nfix, nullptr, nullptr, h0.partial2, h0.C2, h0.ldc2, h0.pw2,
                                   flags & PGCN_SPMM_ACCUMULATE, stream);
    }
    return PGCN_OK;
}

}  // namespace

extern "C" int pgcn_spmm_heads_wide_forward2_f32(const int64_t *rowptr, const int32_t *col, const float *rowstat, const float *s2,
                                                 int64_t lds2, float slope, int32_t mode, int32_t heads, int32_t d, int64_t nrows,
                                                 const int32_t *tasks, int64_t ntasks, const int64_t *seg, int32_t nslices,
                                                 const int32_t *fix, int64_t nfix, const float *B, int64_t ldb, float *C,
                                                 int64_t ldc, float *C2, int64_t ldc2, float *partial_ws,
                                                 int64_t partial_ws_elems, int64_t nslots, uint32_t flags, pgcn_stream_t stream) {
    const Recompute rc{reinterpret_cast<const float4 *>(rowstat), s2, lds2, nrows, slope, mode};
    const Forward2 f2{C2, ldc2, nullptr, heads * d + (heads + 3) / 4 * 4};
    return launch_wide("pgcn_spmm_heads_wide_forward2_f32", rowptr, col, rc, nullptr, &f2, heads, d, nrows, tasks, ntasks, seg,
                       nslices, fix, nfix, B, ldb, C, ldc, partial_ws, partial_ws_elems, nslots, flags, stream);
}

extern "C" int pgcn_spmm_heads_wide_grad_f32(const int64_t *rowptr, const int32_t *col, const float *rowstat, const float *s2,
                                             int64_t lds2, float slope, int32_t mode, int32_t heads, int32_t d, int64_t nrows,
                                             const int32_t *tasks, int64_t ntasks, const int64_t *seg, int32_t nslices,
                                             const int32_t *fix, int64_t nfix, const float *B, int64_t ldb, const float *Z,
                                             int64_t ldz, const float *t, float *C, int64_t ldc, float *de, float *partial_ws,
                                             int64_t partial_ws_elems, int64_t nslots, uint32_t flags, pgcn_stream_t stream) {
    const Recompute rc{reinterpret_cast<const float4 *>(rowstat), s2, lds2, nrows, slope, mode};
    const EdgeGrad eg{Z, ldz, t, de, heads * d + (heads + 3) / 4 * 4};
    return launch_wide("pgcn_spmm_heads_wide_grad_f32", rowptr, col, rc, &eg, nullptr, heads, d, nrows, tasks, ntasks, seg,
                       nslices, fix, nfix, B, ldb, C, ldc, partial_ws, partial_ws_elems, nslots, flags, stream);
}
