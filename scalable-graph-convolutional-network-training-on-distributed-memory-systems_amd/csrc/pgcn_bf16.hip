// pgcn_bf16.hip -- bf16 OPERANDS for the weighted-sum aggregation on gfx950 (MI355X / CDNA4).  include/pgcn_hip.h has the contract.
//
//   cast    Y[r, .]  = bf16(X[r, .])            pgcn_cast_rows_bf16      (rows padded with zeros to a multiple of 8 columns = 16 bytes)
//   pack    out[r, .] = bf16(H[idx[r], .])      pgcn_gather_rows_bf16    (the boundary rows, straight from fp32 H into the send slab)
//   gather  C[i, .] (+)= sum_j a_ij B[j, .]     pgcn_spmm_csr_plan_bf16  (B in bf16; a_ij, the sums, the partial slots and C in fp32)
//
// bf16(.) is round-to-nearest-even on the fp32 bit pattern, in integer arithmetic: u + 0x7fff + bit 16, upper half kept; a NaN becomes
// the quiet NaN 0x7fc0, +-inf and +-0 stay, a finite value above the largest bf16 carries into the exponent and becomes inf -- the bits
// of torch.Tensor.to(torch.bfloat16).
//
// The gather kernel, and why its split is not the fp32 kernel's (pgcn_spmm.hip).  The aggregation is bound by the bytes of the gathered
// rows; a bf16 row is half as long, so the unit that keeps a lane's load at the full 16 bytes is EIGHT features, not four:
//   * a lane owns 8 consecutive features: one global_load_dwordx4 brings them, the even element of a 32-bit word is word << 16, the odd
//     one word & 0xffff0000, then eight fp32 FMAs into eight fp32 accumulators.
//   * a GROUP of LPR = pow2(ceil(f / 8)) <= 64 lanes owns a task (a row, or one <= chunk piece of a long row): f = 128 is 16 lanes and
//     FOUR tasks per wave (the fp32 kernel: 32 lanes, two), so a wave's load instruction still moves 1 KiB and the x8 unroll keeps
//     8 KiB per wave in flight -- the fp32 kernel's bytes, twice its rows.  Wider than 512 features: grid y walks them in passes.
//   * the entries arrive as interleaved {col, value bits} pairs, ONE coalesced non-temporal 8-byte load per lane (they are streamed
//     once and must not evict operand rows from the XCD's L2), parked in 512 B of LDS per wave and broadcast inside the group with
//     ds_read_b128 (two pairs per read); the next batch of pairs is in flight behind the row loads.  Written and read by one wave: no
//     workgroup barrier.
//   * row loads are unpredicated and issued back to back; the surplus places of a ragged batch re-read the task's last row and are
//     selected out (weight and row both zero) before the FMA.
//   * row_map, PGCN_SPMM_ACCUMULATE, the unsliced and the XCD-sliced plan (workgroup b serves slice b % nslices) and the partial slots
//     of cut rows are the fp32 kernel's; the slots hold fp32 sums and go through pgcn_spmm_fixup_f32 in slot order.  No atomics: the
//     same bits from run to run.  A store is clipped at f: the pad columns of B are never written to C.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgcn_internal.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kUnroll = 8;         // row loads of B in flight per batch: 8 x 16 B per lane, 8 KiB per wave
constexpr int kFeat = 8;           // features per lane = one 16-byte load of bf16
constexpr int64_t kMaxLd = (int64_t)1 << 30;   // a row's byte length (2 ld) is held in 32 bits

__device__ __forceinline__ uint32_t bf16_bits(float x) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;          // NaN (torch's conversion: the quiet NaN, sign and payload dropped)
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;                // nearest, ties to even; overflow carries into inf
}

// eight columns from c0 on of one fp32 row -> four packed words; columns at or beyond f are zero
template <bool VEC>
__device__ __forceinline__ uint4 cast8(const float *__restrict__ row, int c0, int f) {
    float x[kFeat];
#pragma unroll
    for (int h = 0; h < kFeat; h += 4) {
        if (VEC && c0 + h + 4 <= f) {
            const float4 v = *reinterpret_cast<const float4 *>(row + c0 + h);
            x[h] = v.x; x[h + 1] = v.y; x[h + 2] = v.z; x[h + 3] = v.w;
        } else {
#pragma unroll
            for (int j = h; j < h + 4; ++j) x[j] = (c0 + j < f) ? row[c0 + j] : 0.f;
        }
    }
    uint4 q;
    q.x = bf16_bits(x[0]) | (bf16_bits(x[1]) << 16);
    q.y = bf16_bits(x[2]) | (bf16_bits(x[3]) << 16);
    q.z = bf16_bits(x[4]) | (bf16_bits(x[5]) << 16);
    q.w = bf16_bits(x[6]) | (bf16_bits(x[7]) << 16);
    return q;
}

// one thread per 16-byte group of an output row; idx == NULL: row r of X, else row idx[r]
template <bool VEC>
__global__ __launch_bounds__(kThreads) void cast_rows_kernel(const float *__restrict__ X, int64_t ldx, const int32_t *__restrict__ idx,
                                                             int64_t nrows, int32_t f, uint16_t *__restrict__ Y, int64_t ldy, int32_t ngr) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t r = t / ngr;
    const int g = (int)(t % ngr);
    if (r >= nrows) return;
    const int64_t src = idx ? (int64_t)idx[r] : r;
    const uint4 q = cast8<VEC>(X + src * ldx, g * kFeat, f);
    *reinterpret_cast<uint4 *>(Y + r * ldy + (int64_t)g * kFeat) = q;
}

int launch_cast(const char *who, const float *X, int64_t ldx, const int32_t *idx, int64_t nrows, int32_t f, uint16_t *Y, int64_t ldy,
                hipStream_t s) {
    if (nrows < 0 || f < 1 || ldx < f || ldy < f) return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes");
    if (ldy % kFeat != 0 || ldy > kMaxLd) return pgcn_set_error2(PGCN_EINVAL, who, "the bf16 leading dimension must be a multiple of 8 below 2^30");
    if (nrows == 0) return PGCN_OK;
    if (!X || !Y) return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    if ((uintptr_t)Y % 16 != 0) return pgcn_set_error2(PGCN_EINVAL, who, "the bf16 matrix must be 16-byte aligned");
    const int32_t ngr = (int32_t)(ldy / kFeat);
    const int64_t blocks = (nrows * ngr + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffLL) return pgcn_set_error2(PGCN_EINVAL, who, "too many rows for one launch");
    const bool vec = (uintptr_t)X % 16 == 0 && ldx % 4 == 0;
    hipLaunchKernelGGL(vec ? cast_rows_kernel<true> : cast_rows_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, s, X, ldx, idx,
                       nrows, f, Y, ldy, ngr);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t swizzle_block(int64_t b, int64_t nb, bool on) {
    if (!on) return b;
    const int64_t per = (nb + 7) / 8;   // block b runs on XCD b % 8: XCD x takes the contiguous range [x * per, (x + 1) * per)
    return (b % 8) * per + b / 8;
}

struct SliceSeg { int64_t v[PGCN_MAX_SLICES + 1]; };

// this lane's 16 bytes of row c of B.  OFF32: every byte offset into B fits 32 bits (uniform 64-bit base + 32-bit lane offset);
// otherwise the row offset is a 64-bit product
template <bool OFF32>
__device__ __forceinline__ uint4 load_row8(const uint16_t *__restrict__ B, uint32_t lane_byte_off, int32_t c, uint32_t row_bytes) {
    const char *p = reinterpret_cast<const char *>(B);
    if constexpr (OFF32) p += (uint32_t)c * row_bytes + lane_byte_off;
    else p += (int64_t)c * (int64_t)row_bytes + lane_byte_off;
    return *reinterpret_cast<const uint4 *>(p);   // default cache policy: the rows are what the L2 is for
}

__device__ __forceinline__ void fma8(float (&acc)[kFeat], float w, const uint4 &q) {
    const uint32_t v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc[2 * j] = fmaf(w, __uint_as_float(v[j] << 16), acc[2 * j]);
        acc[2 * j + 1] = fmaf(w, __uint_as_float(v[j] & 0xffff0000u), acc[2 * j + 1]);
    }
}

// n = min(8, f - fcol) valid columns.  CVEC: p is 16-byte aligned and n is 4 or 8
template <bool CVEC>
__device__ __forceinline__ void load8(float (&x)[kFeat], const float *p, int n) {
    if constexpr (CVEC) {
        const float4 a = *reinterpret_cast<const float4 *>(p);
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
        if (n > 4) {
            const float4 b = *reinterpret_cast<const float4 *>(p + 4);
            x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kFeat; ++j)
            if (j < n) x[j] = p[j];
    }
}

template <bool CVEC>
__device__ __forceinline__ void store8(float *p, const float (&x)[kFeat], int n) {
    if constexpr (CVEC) {
        *reinterpret_cast<float4 *>(p) = make_float4(x[0], x[1], x[2], x[3]);
        if (n > 4) *reinterpret_cast<float4 *>(p + 4) = make_float4(x[4], x[5], x[6], x[7]);
    } else {
#pragma unroll
        for (int j = 0; j < kFeat; ++j)
            if (j < n) p[j] = x[j];
    }
}

// tasks: int4 {kbeg low 32, kbeg high 32, length, dst} (pgcn_spmm_plan_host); dst >= 0: a partial slot, dst < 0: row ~dst.  NULL: one
// task per row.  pairs: uint2 {col, fp32 bits of the value} per stored entry.
template <int LPR, bool OFF32, bool CVEC>
__global__ __launch_bounds__(kThreads, 4) void spmm_bf16_kernel(
    const int64_t *__restrict__ rowptr, const uint64_t *__restrict__ pairs, const int4 *__restrict__ tasks, int64_t ntasks,
    const int32_t *__restrict__ row_map, const uint16_t *__restrict__ B, int64_t ldb, float *__restrict__ C, int64_t ldc, int32_t f,
    float *__restrict__ partial, int64_t nblocks, uint32_t flags, int32_t nslices, SliceSeg seg) {
    constexpr int G = 64 / LPR;
    constexpr int U = (LPR < kUnroll) ? LPR : kUnroll;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int sub = lane % LPR;
    const int gbase = (lane / LPR) * LPR;

    __shared__ __attribute__((aligned(16))) uint2 meta_lds[kWaves][64];
    uint2 *mrow = meta_lds[wave];
    const int fcol = (blockIdx.y * LPR + sub) * kFeat;   // first feature owned by this lane
    int64_t tid, nt;
    if (nslices > 1) {   // workgroup b runs on XCD b % 8 and takes tasks of slice b % nslices only
        const int slice = blockIdx.x % nslices;
        const int64_t sb = blockIdx.x / nslices;
        tid = seg.v[slice] + (sb * kWaves + wave) * G + lane / LPR;
        nt = seg.v[slice + 1];
        if (seg.v[slice] + sb * kWaves * G >= nt) return;
    } else {
        const int64_t bid = swizzle_block(blockIdx.x, nblocks, (flags & PGCN_SPMM_XCD_SWIZZLE) != 0);
        tid = (bid * kWaves + wave) * G + lane / LPR;
        nt = ntasks;
        if (bid * kWaves * G >= nt) return;
    }
    const bool tact = tid < nt;
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
    const bool fact = fcol < f;
    const uint32_t lane_off = (uint32_t)fcol * 2u;
    const uint32_t row_bytes = (uint32_t)(ldb * 2);
    float acc[kFeat];
#pragma unroll
    for (int j = 0; j < kFeat; ++j) acc[j] = 0.f;

    // pairs: one per lane, streamed once -> non-temporal; the loads are unconditional (index clamped into the task; an empty or
    // inactive group reads a harmless valid word of rowptr) so that the next batch stays in flight behind the gathers
    const uint64_t *pp = (len > 0) ? pairs + kbeg : reinterpret_cast<const uint64_t *>(rowptr);
    const int last = (len > 0) ? len - 1 : 0;
    uint64_t np = __builtin_nontemporal_load(pp + ((sub < last) ? sub : last));
    for (int base = 0; __any(base < len); base += LPR) {
        __builtin_amdgcn_wave_barrier();
        mrow[lane] = (len > 0) ? make_uint2((uint32_t)np, (uint32_t)(np >> 32)) : make_uint2(0u, 0u);   // (an empty group: row 0, weight 0)
        __builtin_amdgcn_wave_barrier();
        {
            int e = base + LPR + sub;
            e = (e < last) ? e : last;
            np = __builtin_nontemporal_load(pp + e);
        }
        const int cnt = len - base;   // entries left for this group (may be <= 0)
        const uint2 *mg = mrow + gbase;
#pragma unroll
        for (int k = 0; k < LPR; k += U) {
            if (!__any(k < cnt)) break;
            const bool full = __all(k + U <= cnt);
            int32_t c[U];
            float w[U];
            uint4 x[U];
            if constexpr (U >= 2) {
#pragma unroll
                for (int u = 0; u < U; u += 2) {
                    const uint4 m = *reinterpret_cast<const uint4 *>(mg + k + u);
                    c[u] = (int32_t)m.x; w[u] = __uint_as_float(m.y);
                    c[u + 1] = (int32_t)m.z; w[u + 1] = __uint_as_float(m.w);
                }
            } else {
                const uint2 m = mg[k];
                c[0] = (int32_t)m.x; w[0] = __uint_as_float(m.y);
            }
            if (fact) {
#pragma unroll
                for (int u = 0; u < U; ++u) x[u] = load_row8<OFF32>(B, lane_off, c[u], row_bytes);
                if (!full) {   // the surplus places re-read the task's last row: weight and row out of the sum, whatever they hold
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const bool keep = k + u < cnt;
                        w[u] = keep ? w[u] : 0.f;
                        x[u] = keep ? x[u] : make_uint4(0u, 0u, 0u, 0u);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) fma8(acc, w[u], x[u]);
            }
        }
    }

    if (tact && fact) {
        const int n = (f - fcol < kFeat) ? f - fcol : kFeat;
        if (dst >= 0) {
            store8<CVEC>(partial + (int64_t)dst * f + fcol, acc, n);
        } else {
            const int32_t row = ~dst;
            const int64_t orow = row_map ? row_map[row] : row;
            float *c = C + orow * ldc + fcol;
            if (flags & PGCN_SPMM_ACCUMULATE) {
                float old[kFeat] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                load8<CVEC>(old, c, n);
#pragma unroll
                for (int j = 0; j < kFeat; ++j) acc[j] += old[j];     // (columns at or beyond n are never stored)
            }
            store8<CVEC>(c, acc, n);
        }
    }
}

template <int LPR>
int launch_gather(const int64_t *rowptr, const int32_t *pairs, const int32_t *tasks, int64_t ntasks, const int64_t *seg_host,
                  int32_t nslices, const int32_t *row_map, const uint16_t *B, int64_t ldb, float *C, int64_t ldc, int32_t f,
                  float *partial, uint32_t flags, bool cvec, hipStream_t s) {
    const int64_t per_block = (int64_t)kWaves * (64 / LPR);
    const int ntiles = (f + LPR * kFeat - 1) / (LPR * kFeat);
    SliceSeg seg{};
    int64_t grid;
    if (nslices > 1) {   // every slice gets the blocks of the longest segment
        int64_t longest = 0;
        for (int i = 0; i <= nslices; ++i) seg.v[i] = seg_host[i];
        for (int i = 0; i < nslices; ++i)
            if (seg.v[i + 1] - seg.v[i] > longest) longest = seg.v[i + 1] - seg.v[i];
        grid = ((longest + per_block - 1) / per_block) * nslices;
    } else {
        grid = (ntasks + per_block - 1) / per_block;
        if (flags & PGCN_SPMM_XCD_SWIZZLE) grid = ((grid + 7) / 8) * 8;
    }
    if (grid > 0x7fffffffLL || ntiles > 65535) return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_csr_plan_bf16: too large for one launch");
    const uint64_t *p64 = reinterpret_cast<const uint64_t *>(pairs);
    const int4 *t4 = reinterpret_cast<const int4 *>(tasks);
    const bool off32 = (flags & PGCN_SPMM_OFFSETS32) != 0;
#define PGCN_GO(O32, CV)                                                                                                           \
    hipLaunchKernelGGL((spmm_bf16_kernel<LPR, O32, CV>), dim3((unsigned)grid, ntiles), dim3(kThreads), 0, s, rowptr, p64, t4, ntasks, \
                       row_map, B, ldb, C, ldc, f, partial, grid, flags, nslices, seg)
    if (off32) { if (cvec) PGCN_GO(true, true); else PGCN_GO(true, false); }
    else       { if (cvec) PGCN_GO(false, true); else PGCN_GO(false, false); }
#undef PGCN_GO
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

}  // namespace

extern "C" int pgcn_cast_rows_bf16(const float *X, int64_t ldx, int64_t nrows, int32_t f, uint16_t *Y, int64_t ldy, pgcn_stream_t stream) {
    return launch_cast("pgcn_cast_rows_bf16", X, ldx, nullptr, nrows, f, Y, ldy, (hipStream_t)stream);
}

extern "C" int pgcn_gather_rows_bf16(const float *H, int64_t ldh, const int32_t *idx, int64_t nidx, uint16_t *out, int64_t ldo, int32_t f,
                                     pgcn_stream_t stream) {
    if (nidx > 0 && !idx) return pgcn_set_error(PGCN_EINVAL, "pgcn_gather_rows_bf16: null pointer");
    return launch_cast("pgcn_gather_rows_bf16", H, ldh, idx, nidx, f, out, ldo, (hipStream_t)stream);
}

extern "C" int pgcn_spmm_csr_plan_bf16(const int64_t *rowptr, const int32_t *pairs, const int32_t *tasks, int64_t ntasks,
                                       const int64_t *seg, int32_t nslices, const int32_t *fix, int64_t nfix, const int32_t *row_map,
                                       const uint16_t *B, int64_t ldb, float *C, int64_t ldc, int32_t f, float *partial_ws,
                                       int64_t partial_ws_elems, int64_t nslots, uint32_t flags, pgcn_stream_t stream) {
    if (ntasks < 0 || nfix < 0 || nslots < 0 || f < 1 || ldb < f || ldc < f || nslices < 1 || nslices > PGCN_MAX_SLICES ||
        (nslices > 1 && (!seg || !tasks)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_csr_plan_bf16: bad sizes");
    if (ldb % kFeat != 0)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_csr_plan_bf16: ldb must be a multiple of 8 (every bf16 row starts on 16 bytes)");
    if (ldb > kMaxLd)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_csr_plan_bf16: ldb beyond 2^30: a row's byte length must fit 32 bits");
    if ((uintptr_t)B % 16 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_csr_plan_bf16: B must be 16-byte aligned");
    if (nslices > 1 && (seg[0] != 0 || seg[nslices] != ntasks))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_csr_plan_bf16: seg does not cover the task list");
    if (ntasks == 0) return PGCN_OK;
    const bool own_fixup = nfix > 0 && !(flags & PGCN_SPMM_NO_FIXUP);
    if (!rowptr || !pairs || !B || !C || (own_fixup && (!fix || !tasks)) || (nslots > 0 && (!partial_ws || !tasks)))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_csr_plan_bf16: null pointer");
    if (ntasks > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_csr_plan_bf16: ntasks >= 2^31");
    if ((uintptr_t)pairs % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_csr_plan_bf16: pairs must be 8-byte aligned");
    if (partial_ws_elems < nslots * (int64_t)f)
        return pgcn_set_error(PGCN_ENOMEM, "pgcn_spmm_csr_plan_bf16: partial work-space too small");
    // float4 stores: fcol is a multiple of 8, so with f % 4 == 0 a lane's quads lie wholly inside or wholly outside the row
    const bool cvec = (uintptr_t)C % 16 == 0 && (uintptr_t)partial_ws % 16 == 0 && ldc % 4 == 0 && f % 4 == 0;
    const int nv = (f + kFeat - 1) / kFeat;
    int lpr = 1;
    while (lpr < nv && lpr < 64) lpr *= 2;
    if ((flags & PGCN_SPMM_FPASS64) && lpr > 8) lpr = 8;   // 64 features per pass: grid y walks the passes
    hipStream_t s = (hipStream_t)stream;
    int rc = 1;   // (no shape taken yet)
#define PGCN_CASE(L) \
    if (lpr == L) rc = launch_gather<L>(rowptr, pairs, tasks, ntasks, seg, nslices, row_map, B, ldb, C, ldc, f, partial_ws, flags, cvec, s);
    PGCN_CASE(1) PGCN_CASE(2) PGCN_CASE(4) PGCN_CASE(8) PGCN_CASE(16) PGCN_CASE(32) PGCN_CASE(64)
#undef PGCN_CASE
    if (rc == 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_csr_plan_bf16: no kernel shape");
    if (rc != PGCN_OK || !own_fixup) return rc;
    // the pieces of a cut row: fp32 sums, added in slot order by the sum path's fix-up
    return pgcn_spmm_fixup_f32(fix, nfix, nullptr, row_map, partial_ws, C, ldc, f, flags & PGCN_SPMM_ACCUMULATE, stream);
}
