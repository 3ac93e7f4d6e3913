// pgcn_dense_wide.hip -- the dense products of a layer for widths ABOVE 128 (4 <= fin, fout <= 1024, multiples of 4, one of them
// above 128), on the bf16 matrix cores at fp32 accuracy, fused with what surrounds them exactly as gemm/pgcn_dense.hip and
// gemm/pgcn_wgrad.hip fuse the narrow ones:
//     forward    Y  = [dropout] relu(X . W^T)  (+ the sign mask of Y)
//     backward   Gm = mask ? G * scale : 0,  dX = Gm . W,  dW = Gm^T . X   (Gm formed in registers; written out only when asked for)
// The narrow kernels hold the WHOLE image of W in LDS (96 KB at 128 x 128) and a tile's planes in 96 registers; three bf16 planes of
// a 256 x 256 W are 384 KB.  This family is K-blocked and column-blocked instead.  Arithmetic: the three-plane split of
// pgcn_dense_common.h, the six partial products smallest first, fp32 accumulation in v_mfma_f32_32x32x16_bf16; an element of Y / dX
// is summed over k chunk, k step and partial product in that fixed order, whatever n, the row's position or the grid are.
//
// 1. Image prologue (image_kernel, one workgroup per chunk).  W is split ONCE per product into the chunked B-operand image of
//    pgcn_dense_wide_tile.h in the caller's work-space: chunks of 4 k steps x 4 column blocks (64 x 128 of Bm, 48 KB for the three
//    planes, contiguous), zero outside K x N.  256 x 256: 8 chunks = 384 KB, read by every workgroup and resident in the L2.
//
// 2. Forward / input gradient (wide_kernel<MODE, DROP, RAGGED>), output-stationary.  A 512-thread workgroup owns a PANEL of 256
//    rows, a wave a 32-row tile of it; the workgroup walks the column panels of 128 one after the other (the rows of A are re-read
//    per column panel: 256 x K x 4 B <= 1 MB, an L2 hit).  For one (row panel, column panel) four accumulators (64 registers) stay
//    in place and K is consumed in chunks of 64:
//      * the chunk's 48 KB of image travel from the work-space into a TWO-slot LDS ring (96 KB) by asynchronous global -> LDS
//        copies (global_load_lds_dwordx4, SGPR base + lane offset, as csrc/pgcn_spmm_strip.hip issues them): a wave copies 6 KB =
//        six instructions.  ONE barrier per chunk: behind it every wave's copies of chunk c have landed (s_waitcnt vmcnt(0) before
//        it) and every wave has left the chains of chunk c - 1, so the copies of chunk c + 1 go out into the slot that c - 1 used
//        and fly under the chains of chunk c;
//      * a wave's own pieces of A for chunk c + 1 (8 x 16 B per lane, through the buffer-descriptor windows: rows beyond n read
//        zero, stores beyond n are dropped, no row predicates; pieces of a ragged last chunk beyond K read as zero) are requested
//        at the same point, one chunk ahead, and at the end of chunk c masked + scaled by a SELECT (input gradient: a NaN under a
//        cleared bit gives +0), written out as Gm during the FIRST column panel only, and split into the 48 plane registers;
//      * 4 k steps x 4 column blocks x six MFMAs, the four accumulators interleaved inside a k step (four independent chains).
//    The sequence of chunks runs on across column panels and row panels (persistent workgroups, one per CU), so only the first
//    chunk of a workgroup is not covered.  Epilogue per column panel: ReLU, the keep function of pgcn_dropout.h hashed from (seed,
//    *step, layer, global row id, column) as the narrow kernel does, the sign-mask word per 32 columns by the mask_lanes
//    hand-over, dword stores; columns beyond N are not stored.
//
// 3. Weight gradient (wide_wgrad_kernel + wide_sum_kernel).  The operand layout of pgcn_wgrad.hip (a lane holds one column and eight
//    rows, a step's 32 mask words are one load, Gm = bit ? G * scale : +0 in registers); a wave owns one 64 x 64 tile of dW and one
//    contiguous range of 16-row steps.  Work item = (range, tile), item = range * tiles + tile, eight consecutive items per workgroup
//    (so the waves of a workgroup walk the same rows and share their lines in the L2).  ranges = clamp(2048 / tiles, 1, steps / 4):
//    a function of the shape alone, 2048 waves fill the chip, work-space <= 32 MB (pgcn_dense_wide_tile.h).  Every wave writes its
//    tile of partial matrix `range`; wide_sum_kernel adds the partial matrices in the fixed two-level order of wgrad_sum_kernel (16
//    groups of consecutive partials in order, then the 16 group sums): deterministic, no atomics.
//
// Budget (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, per instantiation; the limit is 256 VGPRs for two waves per SIMD):
//     wide_kernel<0, plain>   VGPRs 179 (ragged 182)   AGPRs 0   scratch 0   LDS 98304 B (dynamic)   occupancy 2 waves / SIMD
//     wide_kernel<0, dropout> VGPRs 186 (ragged 189)   scratch 0
//     wide_kernel<1>          VGPRs 186 (ragged 189)   scratch 0
//     wide_wgrad_kernel       VGPRs 248                scratch 0   LDS 0
//     image_kernel 57, wide_sum_kernel 20
// 96 KB of the CU's 160 KB of LDS: one workgroup = 8 waves = two per SIMD.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <type_traits>

#define PG_HD __device__ __forceinline__

namespace pgcn_dense_wide {

#include "pgcn_dense_tile.h"
#include "pgcn_dense_wide_tile.h"
#define PG_DROPOUT_FN __host__ __device__ __forceinline__
#include "pgcn_dropout.h"

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

template <int I, int N, class F>
PG_HD void static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

PG_HD f32x16 mma(const u32x4 &x, const u32x4 &w, const f32x16 &c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x), __builtin_bit_cast(bf16x8, w), c, 0, 0, 0);
}

// The sign-mask bits of accumulator register R over the wave (pgcn_dense.hip's mask_lanes, restated: that file is not a header).  One
// asm block: the compare -> v_writelane hand-over through VCC needs wait states that the hazard recogniser does not insert around
// inline asm.
template <int R>
PG_HD void mask_lanes(uint32_t &word, float x) {
    asm volatile("v_cmp_nge_f32_e32 vcc, 0, %1\n\ts_nop 4\n\tv_writelane_b32 %0, vcc_lo, %2\n\tv_writelane_b32 %0, vcc_hi, %3"
                 : "+v"(word)
                 : "v"(x), "n"(R), "n"(16 + R)
                 : "vcc");
}

// ---- 1. the image --------------------------------------------------------------------------------------------------------------------
// one workgroup per chunk (np, kc): slot_load on W shifted to the chunk's corner sees a K' x N' matrix whose first 4 x 4 steps and
// blocks are the chunk
__global__ __launch_bounds__(256) void image_kernel(const float *__restrict__ W, int64_t ldw, int transposed, int K, int N, int nkc,
                                                    int vec, char *__restrict__ img) {
    const int chunk = blockIdx.x, np = chunk / nkc, kc = chunk % nkc;
    const int k0 = kChunkK * kc, c0 = kChunkN * np;
    const float *Wc = W + (transposed ? (int64_t)c0 * ldw + k0 : (int64_t)k0 * ldw + c0);
    constexpr int kMine = kChunkSlots / 256;
    float v[kMine][8];
#pragma unroll
    for (int q = 0; q < kMine; ++q) slot_load(Wc, ldw, transposed, K - k0, N - c0, (int)threadIdx.x + 256 * q, v[q], vec != 0);
    char *dst = img + (int64_t)chunk * kChunkBytes;
#pragma unroll
    for (int q = 0; q < kMine; ++q) {
        const int s = (int)threadIdx.x + 256 * q;
        u32x4 p[3];
        const f32x4 lo4 = {v[q][0], v[q][1], v[q][2], v[q][3]}, hi4 = {v[q][4], v[q][5], v[q][6], v[q][7]};
        split8(lo4, hi4, p);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x4 *>(dst + pl * kChunkPlaneBytes + s * 16) = p[pl];
    }
}

// ---- 2. forward / input gradient -----------------------------------------------------------------------------------------------------
struct Args {
    const float *A;            // the streamed operand: X (forward) or G (input gradient), n x K
    int64_t lda;
    const uint32_t *mask_in;   // input gradient: the forward's mask words (n x mask_words(K)), or NULL: every bit set
    float *Gm;                 // input gradient: mask ? G * scale : 0 written out when not NULL (must not overlap A: A is re-read)
    int64_t ldgm;
    uint32_t *mask_out;        // forward: the sign mask of C (n x mask_words(N)) when not NULL
    int64_t n;
    int K, N;
    const char *img;           // the chunked image of Bm (K x N)
    float *C;
    int64_t ldc;
    int relu;
    const int64_t *row_ids;    // dropout: the GLOBAL id of every row (n), or NULL: the row index
    const int64_t *step;       // dropout: the training step, read from device memory at kernel start
    uint64_t seed;
    uint32_t layer, thr;
    float scale;               // dropout forward: 1 / (1 - p); input gradient: what Gm is multiplied by (1 for a plain ReLU layer)
};

struct RowIds {
    uint32_t term, hi;
    bool any_hi;
};

// this wave's 6 KB of a chunk: six asynchronous copies of 64 lanes x 16 B, LDS image lane-linear (M0 = the LDS byte address)
PG_HD void copy_chunk(const char *src, uint32_t dst, uint32_t lane_off) {
#pragma unroll
    for (int q = 0; q < kWaveShare / 1024; ++q)
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                     :: "s"(dst + 1024u * q), "v"(lane_off), "s"(src + 1024 * q) : "memory", "m0");
}

// bit ? g * scale : +0 for piece (ks, h) of a lane (ks: the k step inside the chunk, `word` the mask word of columns 32 (ks >> 1) ..)
PG_HD f32x4 select4(const f32x4 &g, uint32_t word, int ks, int h, int lane, float scale) {
    const uint32_t sh = word >> (16 * (ks & 1) + 8 * (lane >> 5) + 4 * h);
    f32x4 r;
    r.x = (sh & 1u) ? g.x * scale : 0.f; r.y = (sh & 2u) ? g.y * scale : 0.f;
    r.z = (sh & 4u) ? g.z * scale : 0.f; r.w = (sh & 8u) ? g.w * scale : 0.f;
    return r;
}

// C (n x N) = op(A) (n x K) . Bm (K x N).  MODE 0: op(A) = A, C = relu ? max(C, 0) : C (DROP: keep ? that * scale : 0), mask_out = the
// sign (AND keep) words; MODE 1: op(A) = mask_in ? A * scale : 0, written out as Gm when asked for.
template <int MODE, bool DROP, bool RAGGED>
__global__ __launch_bounds__(kThreads, 2) void wide_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) char ring[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n = a.n, npanels = (n + kPanelRows - 1) / kPanelRows;
    const int K = a.K, N = a.N, nkc = chunks_k(K), npn = panels_n(N), mwK = mask_words(K), mwN = mask_words(N);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)ring;
    const uint32_t my_lds = lds0 + (uint32_t)(w * kWaveShare), copy_off = (uint32_t)(lane * 16);

    f32x16 acc[4];
    u32x4 ap[4][3];                                           // bf16 planes of the current chunk's pieces
    f32x4 raw[4][2];                                          // pieces of the next chunk (in flight)
    uint32_t mw2[2] = {~0u, ~0u};                             // their two mask words (MODE 1)

    const uint32_t a_off = piece_lane_offset(a.lda, lane), gm_off = piece_lane_offset(a.ldgm, lane);
    const uint32_t c_off = acc_lane_offset(a.ldc, lane), c_row = (uint32_t)(a.ldc * 4);
    const uint32_t mi_off = (uint32_t)((lane & 31) * mwK * 4);
    const uint32_t mo_off = (uint32_t)(mask_row_of_lane(lane & 31) * mwN * 4);
    const uint32_t no_mask = a.mask_in ? 0u : ~0u;
    auto row0_of = [&](int64_t p) { return p * kPanelRows + (int64_t)w * kRows; };   // (a panel beyond the last: empty windows)

    auto issue_image = [&](int np, int kc, int slot) {
        copy_chunk(a.img + chunk_base(np, kc, nkc) + w * kWaveShare, my_lds + (uint32_t)(slot * kChunkBytes), copy_off);
    };
    auto load_raw = [&](int64_t p, int kc) {
        const window_t wa = tile_window(a.A, a.lda, n, row0_of(p), K);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) load_piece<RAGGED>(raw[ks], wa, a_off, 4 * kc + ks, K, lane);
        if constexpr (MODE == 1) {
            const window_t wm = tile_window(a.mask_in, mwK, a.mask_in ? n : 0, row0_of(p), mwK);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int word = 2 * kc + q;
                const uint32_t x = win_load4u(wm, mi_off + 4u * (uint32_t)(word < mwK ? word : mwK - 1), 0);
                mw2[q] = (word < mwK ? x : 0u) | no_mask;
            }
        }
    };
    // the pieces of chunk (p, np, kc) have landed in raw: mask + scale them, write them out as Gm (first column panel), split them
    auto consume = [&](int64_t p, int np, int kc, bool valid) {
        if constexpr (MODE == 1) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int h = 0; h < 2; ++h) raw[ks][h] = select4(raw[ks][h], mw2[ks >> 1], ks, h, lane, a.scale);
            if (valid && np == 0 && a.Gm) {
                const window_t wgm = tile_window(a.Gm, a.ldgm, n, row0_of(p), K);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) store_piece<RAGGED>(raw[ks], wgm, gm_off, 4 * kc + ks, K, lane);
            }
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) split8(raw[ks][0], raw[ks][1], ap[ks]);
    };

    // dropout (forward): the key once, the row ids of the panel's tile once per row panel, the column's share once per column block
    uint64_t key = 0;
    uint32_t key_hi = 0, dcol = 0;
    RowIds ids{0u, 0u, false};
    if constexpr (DROP && MODE == 0) {
        key = dropout_key(a.seed, (uint64_t)*a.step, a.layer);
        key_hi = (uint32_t)(key >> 32);
    }
    auto load_ids = [&](int64_t p) {
        if constexpr (DROP && MODE == 0) {
            const int64_t r0 = row0_of(p);
            const window_t wi = tile_window(a.row_ids, 1, a.row_ids ? n : 0, r0, 1, 8);
            const uint32_t lo = win_load4u(wi, (uint32_t)(8 * (lane & 31)), 0), hi = win_load4u(wi, (uint32_t)(8 * (lane & 31) + 4), 0);
            const uint64_t own = (uint64_t)r0 + (uint64_t)(lane & 31);
            ids.term = (a.row_ids ? lo : (uint32_t)own) ^ key_hi;
            ids.hi = a.row_ids ? hi : (uint32_t)(own >> 32);          // (any_hi: in the epilogue, when the load has long landed)
        }
    };
    // register r of the lane: tile row (r & 3) + 8 (r >> 2) + 4 hi -- the row's id from the lane that holds it
    auto drop_reg = [&](float x, auto rc) {
        constexpr int r = decltype(rc)::value, R0 = (r & 3) + 8 * (r >> 2);
        const bool up = lane >= 32;
        const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane((int)ids.term, R0), t1 = (uint32_t)__builtin_amdgcn_readlane((int)ids.term, R0 + 4);
        uint32_t u = dropout_fmix32(dcol ^ (up ? t1 : t0));
        if (ids.any_hi) {
            const uint32_t h0 = (uint32_t)__builtin_amdgcn_readlane((int)ids.hi, R0), h1 = (uint32_t)__builtin_amdgcn_readlane((int)ids.hi, R0 + 4);
            const uint32_t h = up ? h1 : h0;
            u = h ? dropout_fmix32(u ^ h) : u;
        }
        return u >= a.thr ? x * a.scale : 0.f;
    };

    auto zero_acc = [&]() {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
    };
    // the chains of one chunk: per k step the B operands of the four column blocks, then six products on each of the four accumulators
    auto chains = [&](int slot) {
        PGCN_DENSE_PRODUCTS;
        const char *img = ring + slot * kChunkBytes;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            u32x4 b[4][3];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) b[nb][pl] = *reinterpret_cast<const u32x4 *>(img + chunk_offset(pl, ks, nb, lane));
#pragma unroll
            for (int j = 0; j < 6; ++j)
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) acc[nb] = mma(ap[ks][kPA[j]], b[nb][kPB[j]], acc[nb]);
        }
    };
    auto epilogue = [&](int64_t p, int np) {
        const window_t wc = tile_window(a.C, a.ldc, n, row0_of(p), N);
        const window_t wmo = tile_window(a.mask_out, mwN, a.mask_out ? n : 0, row0_of(p), mwN);
        if constexpr (DROP && MODE == 0) ids.any_hi = __builtin_amdgcn_ballot_w64(ids.hi != 0u) != 0ull;
        static_for<0, 4>([&](auto nbc) {
            constexpr int nb = decltype(nbc)::value;
            const int nbg = 4 * np + nb;
            if constexpr (DROP && MODE == 0) {
                dcol = dropout_col(key, (uint32_t)(32 * nbg + (lane & 31)));
                static_for<0, 16>([&](auto rc) { acc[nb][decltype(rc)::value] = drop_reg(acc[nb][decltype(rc)::value], rc); });
            }
            store_regs<RAGGED>(acc[nb], 0, 16, nbg, wc, c_off, c_row, N, lane, a.relu);
            if constexpr (MODE == 0) {
                if (a.mask_out) {
                    uint32_t mword = 0;
                    static_for<0, 16>([&](auto rc) { mask_lanes<decltype(rc)::value>(mword, acc[nb][decltype(rc)::value]); });
                    // (bits of columns beyond N come out of zero products: 0 > 0 is false; lanes 32..63 and blocks beyond the mask's
                    //  width aim outside the window)
                    win_store4u(wmo, (lane < 32 && nbg < mwN) ? mo_off + 4u * (uint32_t)nbg : 0xfffffff0u, 0, mword);
                }
            }
        });
    };

    // the sequence of chunks of this workgroup: row panels blockIdx.x, + gridDim.x, ...; per panel the column panels, per column panel
    // the k chunks
    int64_t p = blockIdx.x;
    int np = 0, kc = 0, slot = 0;
    if (p >= npanels) return;                                 // (uniform; the grid never exceeds the panels)
    issue_image(0, 0, 0);
    load_raw(p, 0);
    consume(p, 0, 0, true);
    while (true) {
        int64_t p2 = p;
        int np2 = np, kc2 = kc + 1;
        if (kc2 == nkc) {
            kc2 = 0;
            if (++np2 == npn) {
                np2 = 0;
                p2 += gridDim.x;
            }
        }
        const bool more = p2 < npanels;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's copies of the current chunk have landed ...
        __syncthreads();                                      // ... everybody's have, and nobody reads the other slot any more
        if (more) issue_image(np2, kc2, slot ^ 1);
        load_raw(p2, kc2);                                    // (no more chunks: an empty window, zeros)
        if (np == 0 && kc == 0) load_ids(p);
        if (kc == 0) zero_acc();
        chains(slot);
        if (kc == nkc - 1) epilogue(p, np);
        consume(p2, np2, kc2, more);
        if (!more) break;
        p = p2; np = np2; kc = kc2;
        slot ^= 1;
    }
}

template <int MODE, bool DROP, bool RAGGED>
int launch(const Args &a, int workgroups, hipStream_t s) {
    auto kern = wide_kernel<MODE, DROP, RAGGED>;
    static bool attr_set[64] = {false};
    static std::mutex attr_mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(-1, "hipGetDevice");
    {
        std::lock_guard<std::mutex> lock(attr_mu);
        if (dev < 0 || dev >= 64 || !attr_set[dev]) {
            if (hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kRingBytes) != hipSuccess)
                return fail(-1, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
            if (dev >= 0 && dev < 64) attr_set[dev] = true;
        }
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)workgroups), dim3(kThreads), kRingBytes, s, a);
    return hipGetLastError() == hipSuccess ? 0 : fail(-1, "kernel launch (wide_kernel)");
}

// the image of W into the work-space, then the product
template <int MODE, bool DROP>
int run(Args a, const float *W, int64_t ldw, int transposed, void *ws, hipStream_t s) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0)
        return fail(-1, "hipDeviceGetAttribute(MultiprocessorCount)");
    const int nkc = chunks_k(a.K), npn = panels_n(a.N);
    a.img = static_cast<const char *>(ws);
    hipLaunchKernelGGL(image_kernel, dim3((unsigned)(nkc * npn)), dim3(256), 0, s, W, ldw, transposed, a.K, a.N, nkc,
                       slot_vec_ok(W, ldw, transposed, a.K) ? 1 : 0, static_cast<char *>(ws));
    if (hipGetLastError() != hipSuccess) return fail(-1, "kernel launch (image_kernel)");
    const int64_t npanels = (a.n + kPanelRows - 1) / kPanelRows;
    const int wgs = (int)(npanels < cus ? npanels : cus);     // one persistent workgroup per CU (96 KB of LDS each)
    if (a.K % kChunkK == 0 && a.N % kChunkN == 0) return launch<MODE, DROP, false>(a, wgs, s);
    return launch<MODE, DROP, true>(a, wgs, s);
}

// what the three forward / input-gradient entry points check alike.  K, N: the product's; W is wrows x wcols
inline int check_product(const void *A, int64_t lda, int64_t n, int K, int N, const void *W, int64_t ldw, int wcols, const void *C,
                         int64_t ldc, const void *ws, int64_t ws_bytes) {
    if (n < 0 || !W || (n > 0 && (!A || !C))) return fail(-1, "pgcn_dense_wide: bad argument");
    if (n > ((int64_t)1 << 40)) return fail(-1, "pgcn_dense_wide: n out of range");
    if (ldw < wcols || ldc < N) return fail(-1, "pgcn_dense_wide: leading dimension below the width");
    if (int rc = check_streamed(A, lda, K)) return rc;
    if (int rc = check_ld(ldc)) return rc;
    if (n > 0 && (!ws || (uintptr_t)ws % 16 || ws_bytes < image_bytes(K, N)))
        return fail(-2, "pgcn_dense_wide: the image work-space is too small or not 16-byte aligned");
    return 0;
}

// ---- 3. the weight gradient ----------------------------------------------------------------------------------------------------------
constexpr int kDepth = 3;                 // steps of operands in flight (register sets of 33)
constexpr int kGroups = 16;               // wide_sum_kernel: groups of consecutive partial matrices

struct StepRaw {                          // one lane and step: operand blocks (a0, a1 of G; b0, b1 of X) x 8 rows, the step's mask word
    float a[2][8], b[2][8];
    uint32_t m;
};
using rsrc_t = __amdgpu_buffer_rsrc_t;
PG_HD float buf_load(rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}
// WGUARD: ragged widths -- a lane whose column lies beyond the width reads a clamped column and drops the value
template <bool WGUARD>
PG_HD void load_step(StepRaw &s, rsrc_t g, rsrc_t x, uint32_t soff_g, uint32_t soff_x, const uint32_t (&goff)[8], const uint32_t (&xoff)[8],
                     bool a0_ok, bool a1_ok, bool b0_ok, bool b1_ok, rsrc_t m, uint32_t moff, uint32_t soff_m) {
    s.m = __builtin_bit_cast(uint32_t, buf_load(m, moff, soff_m));
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        s.a[0][j] = buf_load(g, goff[j], soff_g);
        s.a[1][j] = buf_load(g, goff[j] + ((!WGUARD || a1_ok) ? 128u : 0u), soff_g);
        s.b[0][j] = buf_load(x, xoff[j], soff_x);
        s.b[1][j] = buf_load(x, xoff[j] + ((!WGUARD || b1_ok) ? 128u : 0u), soff_x);
        if constexpr (WGUARD) {
            s.a[0][j] = a0_ok ? s.a[0][j] : 0.f;
            s.a[1][j] = a1_ok ? s.a[1][j] : 0.f;
            s.b[0][j] = b0_ok ? s.b[0][j] : 0.f;
            s.b[1][j] = b1_ok ? s.b[1][j] : 0.f;
        }
    }
}
// Gm of one step in place: the 64 select bits of register j and block b are word (row j, b) for lanes 0-31 and word (row 8 + j, b) for
// lanes 32-63 of the one mask load (lane l & 31 holds word (row l & 15, block l >> 4)): two v_readlane and one select on the pair
PG_HD void mask_step(StepRaw &s, float scale, uint32_t all_set) {
    const uint32_t w = s.m | all_set;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)w, 16 * b + j), hi = (uint32_t)__builtin_amdgcn_readlane((int)w, 16 * b + 8 + j);
            s.a[b][j] = __builtin_amdgcn_inverse_ballot_w64(((uint64_t)hi << 32) | lo) ? s.a[b][j] * scale : 0.f;
        }
}
PG_HD void planes_of(const float (&v)[8], u32x4 (&p)[3]) {
    const f32x4 lo4 = {v[0], v[1], v[2], v[3]}, hi4 = {v[4], v[5], v[6], v[7]};
    split8(lo4, hi4, p);
}
PG_HD void step_product(const StepRaw &s, f32x16 (&acc)[2][2]) {
    PGCN_DENSE_PRODUCTS;
    u32x4 a0[3], a1[3], b0[3], b1[3];
    planes_of(s.a[0], a0);
    planes_of(s.b[0], b0);
    planes_of(s.b[1], b1);
    planes_of(s.a[1], a1);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        acc[0][0] = mma(a0[kPA[i]], b0[kPB[i]], acc[0][0]);
        acc[0][1] = mma(a0[kPA[i]], b1[kPB[i]], acc[0][1]);
        acc[1][0] = mma(a1[kPA[i]], b0[kPB[i]], acc[1][0]);
        acc[1][1] = mma(a1[kPA[i]], b1[kPB[i]], acc[1][1]);
    }
}

// partial[range][FO x FI] (FO = 64 TO, FI = 64 TK): this wave's 64 x 64 tile over its row range
template <bool WGUARD>
__global__ __launch_bounds__(kThreads, 2) void wide_wgrad_kernel(const float *__restrict__ G, int64_t ldg, const float *__restrict__ X,
                                                                 int64_t ldx, int64_t n, int fout, int fin, float *__restrict__ partial,
                                                                 const uint32_t *__restrict__ mask, float scale, int TO, int TK, int ranges) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tiles = TO * TK;
    const int item = (int)blockIdx.x * kWaves + w;
    if (item >= tiles * ranges) return;                       // (no barrier in this kernel)
    const int range = item / tiles, tile = item % tiles;
    const int to = tile / TK, tk = tile % TK;
    const int lo = lane & 31, hi = lane >> 5;
    const int FI = 64 * TK, FO = 64 * TO;
    const int64_t nsteps = (n + kStepRows - 1) / kStepRows;
    const int64_t s0 = nsteps * range / ranges, s1 = nsteps * (range + 1) / ranges;
    const int ocol = 64 * to + lo, kcol = 64 * tk + lo;
    const bool a0_ok = ocol < fout, a1_ok = ocol + 32 < fout, b0_ok = kcol < fin, b1_ok = kcol + 32 < fin;
    uint32_t goff[8], xoff[8];
    {
        const int oc = a0_ok ? ocol : fout - 1, kc = b0_ok ? kcol : fin - 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            goff[j] = (uint32_t)(((int64_t)(8 * hi + j) * ldg + oc) * 4);
            xoff[j] = (uint32_t)(((int64_t)(8 * hi + j) * ldx + kc) * 4);
        }
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // the wave's row range as buffers: base = first row of the range, size = what is left of the matrix (clipped to a descriptor's 32
    // bits: the host checked that a range's own bytes fit); rows beyond n read as zero
    const int64_t gstep = (int64_t)kStepRows * ldg * 4, xstep = (int64_t)kStepRows * ldx * 4;
    auto descriptor = [&](const void *M, int64_t ld, int64_t step_bytes) -> rsrc_t {
        const int64_t first = s0 * kStepRows;
        int64_t bytes = (n - first) * ld * 4;
        if (bytes > 0xfffff000LL) bytes = 0xfffff000LL;
        if (bytes < 0 || !M) bytes = 0;
        const uint64_t base = (uint64_t)(reinterpret_cast<const char *>(M) + s0 * step_bytes);
        const uint32_t blo = __builtin_amdgcn_readfirstlane((uint32_t)base), bhi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
        const uint32_t nb = __builtin_amdgcn_readfirstlane((uint32_t)bytes);
        return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((uint64_t)bhi << 32) | blo), 0, (int)nb, 0x00020000);
    };
    const rsrc_t gr = descriptor(G, ldg, gstep), xr = descriptor(X, ldx, xstep);
    const uint32_t gs = (uint32_t)gstep, xs = (uint32_t)xstep;
    const int mw = (fout + 31) >> 5;
    const rsrc_t mr = descriptor(mask, mw, (int64_t)kStepRows * mw * 4);      // (no mask: empty, zero words OR-ed with all_set)
    const uint32_t ms = (uint32_t)(kStepRows * mw * 4), all_set = mask ? 0u : ~0u;
    uint32_t moff;
    {
        const int word = 2 * to + ((lane >> 4) & 1);
        moff = (uint32_t)(((lane & 15) * mw + (word < mw ? word : mw - 1)) * 4);
    }
    const int nst = __builtin_amdgcn_readfirstlane((int)(s1 - s0));
    {
        StepRaw raw[kDepth];
#pragma unroll
        for (int d = 0; d < kDepth; ++d)
            if (d < nst) load_step<WGUARD>(raw[d], gr, xr, d * gs, d * xs, goff, xoff, a0_ok, a1_ok, b0_ok, b1_ok, mr, moff, d * ms);
        int t = 0;
        uint32_t og = kDepth * gs, ox = kDepth * xs, om = kDepth * ms;
        while (t + kDepth <= nst) {
#pragma unroll
            for (int d = 0; d < kDepth; ++d) {
                mask_step(raw[d], scale, all_set);
                step_product(raw[d], acc);
                if (t + d + kDepth < nst)
                    load_step<WGUARD>(raw[d], gr, xr, og + d * gs, ox + d * xs, goff, xoff, a0_ok, a1_ok, b0_ok, b1_ok, mr, moff, om + d * ms);
            }
            t += kDepth;
            og += kDepth * gs;
            ox += kDepth * xs;
            om += kDepth * ms;
        }
#pragma unroll
        for (int d = 0; d < kDepth; ++d)
            if (t + d < nst) {
                mask_step(raw[d], scale, all_set);
                step_product(raw[d], acc);
            }
    }
    // accumulator register r of lane (lo, hi), block (i, j) of the tile = element (64 to + 32 i + (r & 3) + 8 (r >> 2) + 4 hi,
    // 64 tk + 32 j + lo) of partial matrix `range` (every element of the padded FO x FI matrix is written: zeros beyond the widths)
    float *out = partial + (int64_t)range * FO * FI;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = 64 * to + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * hi, k = 64 * tk + 32 * j + lo;
                out[o * FI + k] = acc[i][j][r];
            }
}

// dW[o][k] = sum over the partial matrices, as kGroups sums of consecutive partials (each in order) added in group order: the order of
// pgcn_wgrad.hip's wgrad_sum_kernel.  Thread (e, g): four consecutive k of one o, group g; block = 16 chunks x 16 groups.
__global__ __launch_bounds__(256) void wide_sum_kernel(const float *__restrict__ partial, int parts, int FO, int FI, int fout, int fin,
                                                       float *__restrict__ dW, int64_t lddw) {
    __shared__ f32x4 part[16][kGroups + 1];
    const int g = threadIdx.x & (kGroups - 1), c = threadIdx.x >> 4;
    const int chunk = blockIdx.x * 16 + c;
    const int per = (parts + kGroups - 1) / kGroups;
    const int p0 = g * per, p1 = (p0 + per < parts) ? p0 + per : parts;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (chunk * 4 < FO * FI) {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(partial) + chunk;
        const int64_t slab = (int64_t)FO * FI / 4;
        for (int p = p0; p < p1; ++p) s = s + src[(int64_t)p * slab];
    }
    part[c][g] = s;
    __syncthreads();
    if (g == 0 && chunk * 4 < FO * FI) {
        f32x4 t = part[c][0];
#pragma unroll
        for (int q = 1; q < kGroups; ++q) t = t + part[c][q];
        const int o = (chunk * 4) / FI, k = (chunk * 4) % FI;
        if (o < fout) {
            float *dst = dW + (int64_t)o * lddw + k;
            if (k + 0 < fin) dst[0] = t.x;
            if (k + 1 < fin) dst[1] = t.y;
            if (k + 2 < fin) dst[2] = t.z;
            if (k + 3 < fin) dst[3] = t.w;
        }
    }
}

}  // namespace pgcn_dense_wide

// ---- the C ABI (include/pgcn_dense_wide.h) -------------------------------------------------------------------------------------------
extern "C" int pgcn_dense_wide_abi_version(void) { return 1; }
extern "C" const char *pgcn_dense_wide_last_error(void) { return pgcn_dense_wide::g_err; }

extern "C" int64_t pgcn_wide_image_ws_bytes(int32_t K, int32_t N) {
    if (K <= 0 || N <= 0) return 0;
    return pgcn_dense_wide::image_bytes(K, N);
}

extern "C" int pgcn_wide_linear_relu_f32(const float *X, int64_t ldx, int64_t n, int32_t fin, const float *W, int64_t ldw, int32_t fout,
                                         float *Y, int64_t ldy, int32_t relu, uint32_t *mask, const int64_t *row_ids, uint64_t seed,
                                         const int64_t *step, uint32_t layer, uint32_t thr, void *ws, int64_t ws_bytes, void *stream) {
    using namespace pgcn_dense_wide;
    if (int rc = check_widths(fin, fout)) return rc;
    if (int rc = check_product(X, ldx, n, fin, fout, W, ldw, fin, Y, ldy, ws, ws_bytes)) return rc;
    if (step && row_ids && (uintptr_t)row_ids % 8) return fail(-2, "pgcn_dense_wide: row_ids must be 8-byte aligned");
    if ((uintptr_t)mask % 4) return fail(-2, "pgcn_dense_wide: the mask words must be 4-byte aligned");
    if (n == 0) return 0;
    Args a{};
    a.A = X; a.lda = ldx; a.mask_out = mask; a.n = n; a.K = fin; a.N = fout; a.C = Y; a.ldc = ldy;
    a.relu = (relu || step) ? 1 : 0;
    if (!step) return run<0, false>(a, W, ldw, 1, ws, (hipStream_t)stream);
    a.row_ids = row_ids; a.step = step; a.seed = seed; a.layer = layer; a.thr = thr; a.scale = dropout_scale(thr);
    return run<0, true>(a, W, ldw, 1, ws, (hipStream_t)stream);
}

extern "C" int pgcn_wide_grad_input_f32(const float *G, int64_t ldg, const uint32_t *mask, float scale, float *Gm, int64_t ldgm, int64_t n,
                                        int32_t fout, const float *W, int64_t ldw, int32_t fin, float *dX, int64_t lddx, void *ws,
                                        int64_t ws_bytes, void *stream) {
    using namespace pgcn_dense_wide;
    if (int rc = check_widths(fin, fout)) return rc;
    if (int rc = check_product(G, ldg, n, fout, fin, W, ldw, fin, dX, lddx, ws, ws_bytes)) return rc;
    if (Gm) {
        if (int rc = check_streamed(Gm, ldgm, fout)) return rc;
        if (Gm == G) return fail(-1, "pgcn_dense_wide: Gm must not be G (the rows of G are read once per column panel)");
    }
    if ((uintptr_t)mask % 4) return fail(-2, "pgcn_dense_wide: the mask words must be 4-byte aligned");
    if (n == 0) return 0;
    Args a{};
    a.A = G; a.lda = ldg; a.mask_in = mask; a.Gm = Gm; a.ldgm = ldgm; a.n = n; a.K = fout; a.N = fin; a.C = dX; a.ldc = lddx;
    a.relu = 0; a.scale = scale;
    return run<1, false>(a, W, ldw, 0, ws, (hipStream_t)stream);
}

extern "C" int64_t pgcn_wide_weight_grad_ws_elems(int64_t n, int32_t fout, int32_t fin) {
    using namespace pgcn_dense_wide;
    if (n <= 0 || fout <= 0 || fin <= 0) return 0;
    return (int64_t)wgrad_ranges(n, fout, fin) * (64 * wgrad_tiles(fout)) * (64 * wgrad_tiles(fin));
}

extern "C" int pgcn_wide_weight_grad_f32(const float *G, int64_t ldg, const uint32_t *mask, float scale, const float *X, int64_t ldx,
                                         int64_t n, int32_t fout, int32_t fin, float *dW, int64_t lddw, float *ws, int64_t ws_elems,
                                         void *stream) {
    using namespace pgcn_dense_wide;
    if (int rc = check_widths(fin, fout)) return rc;
    if (n < 0 || !dW || (n > 0 && (!G || !X))) return fail(-1, "pgcn_wide_weight_grad_f32: bad argument");
    if (ldg < fout || ldx < fin || lddw < fin) return fail(-1, "pgcn_wide_weight_grad_f32: leading dimension below the width");
    if (n > ((int64_t)1 << 40)) return fail(-1, "pgcn_wide_weight_grad_f32: n out of range");
    if (check_ld(ldg) || check_ld(ldx)) return -2;
    if ((uintptr_t)mask % 4 || (uintptr_t)G % 4 || (uintptr_t)X % 4)
        return fail(-2, "pgcn_wide_weight_grad_f32: operands and mask words must be 4-byte aligned");
    if (n == 0) return 0;
    const int TO = wgrad_tiles(fout), TK = wgrad_tiles(fin), ranges = wgrad_ranges(n, fout, fin), FO = 64 * TO, FI = 64 * TK;
    if (!ws || (uintptr_t)ws % 16 || ws_elems < (int64_t)ranges * FO * FI)
        return fail(-2, "pgcn_wide_weight_grad_f32: work-space too small or not 16-byte aligned");
    {
        const int64_t steps = (n + kStepRows - 1) / kStepRows, per = steps / ranges + 2;
        if (per * kStepRows * (ldg > ldx ? ldg : ldx) * 4 >= ((int64_t)1 << 31))
            return fail(-2, "pgcn_wide_weight_grad_f32: a row range exceeds the 32-bit range of a buffer descriptor");
    }
    hipStream_t s = (hipStream_t)stream;
    const int items = TO * TK * ranges, wgs = (items + kWaves - 1) / kWaves;
    const bool ragged = fout % 64 != 0 || fin % 64 != 0;
    if (ragged)
        hipLaunchKernelGGL(wide_wgrad_kernel<true>, dim3((unsigned)wgs), dim3(kThreads), 0, s, G, ldg, X, ldx, n, fout, fin, ws, mask, scale, TO,
                           TK, ranges);
    else
        hipLaunchKernelGGL(wide_wgrad_kernel<false>, dim3((unsigned)wgs), dim3(kThreads), 0, s, G, ldg, X, ldx, n, fout, fin, ws, mask, scale,
                           TO, TK, ranges);
    if (hipGetLastError() != hipSuccess) return fail(-1, "kernel launch (wide_wgrad_kernel)");
    const int chunks = FO * FI / 4;
    hipLaunchKernelGGL(wide_sum_kernel, dim3((unsigned)((chunks + 15) / 16)), dim3(256), 0, s, ws, ranges, FO, FI, fout, fin, dW, lddw);
    return hipGetLastError() == hipSuccess ? 0 : fail(-1, "kernel launch (wide_sum_kernel)");
}
