// pgcn_spmm_strip.hip -- LDS-staged SpMM over TALL tiles (512 rows x 128 columns) for gfx950.
//
// Why.  A gather through the vector L1 moves one 512 B row of the dense operand per stored entry and saturates
// near 18 TB/s on an MI355X even when every row hits in L2 (r02 probe, uniform hot set): at 58.8 GB of gathers per
// Reddit-sized SpMM that is the whole budget.  Staging a 128-row panel of B once in LDS (64 KB through the same L1
// path) and serving all entries of a 512-row tile from LDS replaces 512 B per ENTRY by 64 KB per TILE (part of
// /root/reference/GPU/PGCN.py:127's torch.sparse.mm).
//
// Records.  A RECORD is one LAYER of a 512 x 128 tile: the (2 l)-th and (2 l + 1)-th stored entry of every row,
// i.e. exactly 2 {byte offset of the column's row in the staged panel, value} pairs per row = 8 KB; an unused slot
// points at an all-zero LDS row with value 0.0 (no row the matrix does not reference is ever combined: no 0 x Inf).
// With a fixed shape the compute phase is straight-line code: no counts, no branches.
//
// Mapping (second generation, r02; tools/micro/lds_rate.hip and tools/micro/strip_bench.cpp are the measurements):
//   * the LDS serves whole-row reads at 232 B/clk/CU, but a ds_read_b128 that BROADCASTS 16 B of pairs to a group
//     costs as much as one that reads 1 KB of rows.  A GROUP is 16 lanes and a lane owns 8 features (chunks s and
//     s + 16 of the 32 float4 chunks of a row), so one pair read serves FOUR groups (4 x 2 entries) and is followed
//     by eight row reads: pairs take 1/5 of the LDS cycles (1/3 with 32-lane groups).  Lanes of a ds_read_b128
//     phase group ({0-3,12-15,20-27}, ...) read chunk (lane mod 16) of their rows -- the bank pattern of a linear
//     read: conflict-free for any mix of rows.  64 groups x 8 row slots: local row = j * 64 + g, 8 x 2 float4
//     accumulators per lane over the whole piece.
//   * pairs are wave-private: wave w copies the 512 B of its four groups (global_load_lds, lanes 0-31; lane 32
//     brings the next record's 16-byte header) into its own three-slot ring two records ahead and waits for them
//     with a counted vmcnt -- no barrier, no scalar loads in the loop (an outstanding s_load sits in lgkmcnt behind
//     every counted LDS wait).
//   * a workgroup barrier is only needed when the PANEL changes (every ~3 records on the benchmark graph): one per
//     run of records that share a panel.  The next run's panel is copied into the other buffer during the current
//     run; its four copies per thread go out BETWEEN the compute steps of the run's first record (SGPR-base form,
//     no address registers), not in a burst behind the barrier.
//   * LDS reads are inline asm with hand-counted lgkmcnt (a ds_read the compiler can see makes it wait for ALL
//     outstanding asynchronous copies); sched_barrier pins "next slot's reads before this slot's FMAs".
// Deterministic: fixed order, no atomics; a piece writes 512 partial rows to slots that pgcn_spmm_fixup_f32 adds
// in list order.  Bit-identical to the first-generation kernel on the same records (strip_bench.cpp), 1.27x faster.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "pgcn_device.h"
#include "pgcn_internal.h"
#include "pgcn_once.h"
#include "pgcn_strip_map.h"

#pragma clang diagnostic ignored "-Winline-asm"   // the copies set M0 themselves ("m0" on the clobber list)

namespace {

constexpr int TRS = PGCN_STRIP_TR;     // 512 rows per strip tile
constexpr int TC = PGCN_CORE_TC;       // 128 columns per panel
constexpr int SB = PGCN_STRIP_B;       // pair slots per row and record
constexpr int kThreads = 1024;
constexpr int NG = kThreads / 16;      // 64 groups of 16 lanes
constexpr int RW = TRS / NG;           // 8 row slots per group: local row = j * 64 + g
static_assert(RW == 8 && NG == 64 && SB == 2, "layout constants are baked into the record format");

constexpr int kPanelBytes = (TC + 1) * 512;           // 128 rows x 128 fp32 + the all-zero row
constexpr int kPadOff = TC * 512;                     // what an unused pair slot points at
constexpr int kRecBytes = TRS * SB * 8;               // 8 KB of pairs per record
constexpr int kWaveRec = kRecBytes / (kThreads / 64); // 512 B: the pairs of one wave's four groups
constexpr int kRing = 3;                              // ring slots per wave (record k, k + 1, k + 2)
constexpr int kSlotBytes = kWaveRec + 16;             // ... each followed by the record's 16-byte header
constexpr int kOffRing = 2 * kPanelBytes;
constexpr int kSmem = kOffRing + (kThreads / 64) * kRing * kSlotBytes;
static_assert(kSmem <= 160 * 1024, "LDS budget of one CU");
// The panel copies add ONE 32-bit per-lane byte offset to a 64-bit wave-uniform base: lane_off = ((tid >> 5) * ldb + c4s * 4) * 4
// with tid >> 5 <= kThreads / 32 - 1 = 31 and c4s <= 31.  It fits 32 bits while 31 * ldb + 124 <= 2^30 - 1, i.e. ldb <= 34 636 829
// floats; the entry points refuse a wider operand (both kernels and the generic ones, so the answer does not depend on alignment).
constexpr int64_t kMaxLdb = ((int64_t{1} << 30) - 1 - 31 * 4) / (kThreads / 32 - 1);
static_assert((((int64_t)(kThreads / 32 - 1) * kMaxLdb + 31 * 4) * 4) <= 0xffffffffLL &&
              (((int64_t)(kThreads / 32 - 1) * (kMaxLdb + 1) + 31 * 4) * 4) > 0xffffffffLL, "largest ldb whose lane offset fits 32 bits");

// Every LDS address below comes from pgcn_strip_map.h (evaluated on the host by tests/native/pgcn_strip_map_host.cpp); the constants
// above are its 16-wave values, which the value-free kernel shares.
template <int NW> using Map = pgcn_strip_map::Map<NW>;
static_assert(Map<16>::kThreads == kThreads && Map<16>::kWaveRec == kWaveRec && Map<16>::kSlotBytes == kSlotBytes &&
              Map<16>::kSmem == kSmem && pgcn_strip_map::kPanelBytes == kPanelBytes && pgcn_strip_map::kPadOff == kPadOff &&
              pgcn_strip_map::kOffRing == kOffRing && pgcn_strip_map::kRing == kRing && pgcn_strip_map::kGroupBytes == RW * SB * 8,
              "pgcn_strip_map.h and the record format disagree");
// The 8-wave form (512 threads, pgcn_spmm_strip_w8_f32): the same records, work list, panels and slots in half the wave slots and
// ~70 % of the registers of a CU, so that the gather part's workgroups (2 KB of LDS each) run BESIDE a strip workgroup when the
// two are launched on two lanes (tuning.lanes) instead of time-slicing the CUs with it.  Wave W takes what waves 2 W and 2 W + 1
// of the 16 take: 16 row slots, the eight steps of compute_record twice (PASS 1: + 512 B into the ring slot, the other half of the
// accumulators).  Per row the same entries in the same order: the partial rows are those of the 16-wave kernel bit for bit.
// Its lane offsets of the panel copies use tid >> 5 <= 15: kMaxLdb (the 16-wave bound) covers them.

typedef __attribute__((address_space(1))) const void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;

using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// wait until at most n of this wave's asynchronous copies are outstanding (n is wave-uniform).  The largest count a wave asks for is
// two panels' and two ring slots' copies behind the awaited one: 4 + 4 + 1 + 1 = 10 with 16 waves, 8 + 8 + 2 + 2 = 20 with 8; anything
// larger waits for that many (stricter, still correct).  s_waitcnt takes an immediate, hence one case per count.
#define PGCN_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define PGCN_VMCNT_CASE(n) case n: PGCN_VMCNT(n); break;
#define PGCN_VMCNT_CASES_0_9 PGCN_VMCNT_CASE(0) PGCN_VMCNT_CASE(1) PGCN_VMCNT_CASE(2) PGCN_VMCNT_CASE(3) PGCN_VMCNT_CASE(4) \
                             PGCN_VMCNT_CASE(5) PGCN_VMCNT_CASE(6) PGCN_VMCNT_CASE(7) PGCN_VMCNT_CASE(8) PGCN_VMCNT_CASE(9)
#define PGCN_VMCNT_CASES_10_19 PGCN_VMCNT_CASE(10) PGCN_VMCNT_CASE(11) PGCN_VMCNT_CASE(12) PGCN_VMCNT_CASE(13) PGCN_VMCNT_CASE(14) \
                               PGCN_VMCNT_CASE(15) PGCN_VMCNT_CASE(16) PGCN_VMCNT_CASE(17) PGCN_VMCNT_CASE(18) PGCN_VMCNT_CASE(19)
template <int NW>
__device__ __forceinline__ void wait_vm_dyn(int n) {
    static_assert(2 * Map<NW>::kPanelCopies + 2 * Map<NW>::kPairCopies == (NW == 16 ? 10 : 20), "the default case is the largest count");
    if constexpr (NW == 16) {
        switch (__builtin_amdgcn_readfirstlane(n)) { PGCN_VMCNT_CASES_0_9 default: PGCN_VMCNT(10); break; }
    } else {
        switch (__builtin_amdgcn_readfirstlane(n)) { PGCN_VMCNT_CASES_0_9 PGCN_VMCNT_CASES_10_19 default: PGCN_VMCNT(20); break; }
    }
}
#undef PGCN_VMCNT_CASES_10_19
#undef PGCN_VMCNT_CASES_0_9
#undef PGCN_VMCNT_CASE
#undef PGCN_VMCNT

// LDS reads the compiler does not see as memory operations (a visible ds_read makes it wait for ALL outstanding
// asynchronous copies); the matching waits take the results as read-write operands.
template <int OFF>
__device__ __forceinline__ void lds_read_b128(f32x4 &v, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
}
__device__ __forceinline__ void lds_wait0(f32x4 &a, f32x4 &b, f32x4 &c, f32x4 &d, f32x4 &e) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e));
}
__device__ __forceinline__ void lds_wait0_4(f32x4 &a, f32x4 &b, f32x4 &c, f32x4 &d) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
__device__ __forceinline__ void lds_wait1(f32x4 &a) {
    asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(a));
}

// The lane id, recomputed where it is needed: the 8-wave kernel has 128 accumulators and 44 registers of LDS data in flight, and only
// four more fit under 176 (two strip waves + two gather waves per SIMD), so nothing derived from the thread id stays live across the
// record loop but the lane offset of the panel copies (volatile: not hoisted out of the loop again)
__device__ __forceinline__ int lane_id_here() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
__device__ __forceinline__ void add_uniform(uint32_t &v, int d) {   // v += d in place (d wave-uniform): no second register for the sum
    asm volatile("v_add_u32 %0, %1, %0" : "+v"(v) : "s"(__builtin_amdgcn_readfirstlane(d)));
}

// 4 asynchronous copies per thread: the 128 rows of a panel, 16 B per lane, LDS image lane-linear
// Asynchronous copies Q0..Q1-1 (of 4 per thread) of a panel: 128 rows x 512 B, 16 B per lane, LDS image lane-linear.
// Source = (wave-uniform 64-bit base of the quarter panel) + (one 32-bit per-lane offset, the same for every panel):
// the SGPR-base form of global_load_lds, so a copy issued between the compute steps needs no address registers.
// The LAST panel of an operand whose row count is not a multiple of 128 is the window [ncols - 128, ncols): the
// host stores its pair offsets relative to that base, no copy ever reads past the operand.
template <int Q0, int Q1, int NW = 16>
__device__ __forceinline__ void issue_panel(int panel, uint32_t lds0, int pb, const float *__restrict__ B, int64_t ldb,
                                            int64_t ncols, int fcol0, uint32_t lane_off, int wave) {
    int64_t col0 = (int64_t)panel * TC;
    col0 = col0 + TC <= ncols ? col0 : ncols - TC;
#pragma unroll
    for (int q = Q0; q < Q1; ++q) {
        const char *base = reinterpret_cast<const char *>(B + (col0 + Map<NW>::panel_src_row(q)) * ldb + fcol0);   // wave-uniform
        const uint32_t dst = Map<NW>::panel_dst(lds0, pb, q, wave);                                              // wave-uniform
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                     :: "s"(dst), "v"(lane_off), "s"(base) : "memory", "m0");
    }
}

// One of the four copies, skipped when `on` (wave-uniform) is 0.  The branch lives INSIDE the asm statement: a C++
// branch between the compute steps splits the straight-line block of 40 hand-scheduled LDS reads and the register
// allocator gives up (100+ spills).
template <int Q, int NW = 16>
__device__ __forceinline__ void issue_panel_if(int on, int panel, uint32_t lds0, int pb, const float *__restrict__ B, int64_t ldb,
                                               int64_t ncols, int fcol0, uint32_t lane_off, int wave) {
    int64_t col0 = (int64_t)panel * TC;
    // 8 waves: the same window by a 32-bit compare -- for every int panel, panel < ncols / 128 (floor) is (panel + 1) * 128 <= ncols, and a
    // quotient beyond 2^31 - 1 exceeds every panel (the 64-bit compare runs on the vector ALU: two registers at the kernel's tightest point)
    if constexpr (NW == 8)
        col0 = panel < (int)min(ncols / TC, (int64_t)0x7fffffff) ? col0 : ncols - TC;
    else
        col0 = col0 + TC <= ncols ? col0 : ncols - TC;
    const char *base = reinterpret_cast<const char *>(B + (col0 + Map<NW>::panel_src_row(Q)) * ldb + fcol0);
    const uint32_t dst = Map<NW>::panel_dst(lds0, pb, Q, wave);
    asm volatile("s_cmp_eq_u32 %3, 0\n\ts_cbranch_scc1 1f\n\ts_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n1:"
                 :: "s"(__builtin_amdgcn_readfirstlane(dst)), "v"(lane_off), "s"(base), "s"(__builtin_amdgcn_readfirstlane(on)) : "memory", "m0", "scc");
}

// 1 asynchronous copy per wave into ring slot `slot`: lanes 0-31 the pairs of this wave's four groups of record k,
// lane 32 the header of record k + 1 (so the loop needs no scalar loads: an outstanding s_load would sit in lgkmcnt
// behind every counted LDS wait, and a header line missing the scalar cache stalls all 16 waves)
// 8 waves: 1 KB of pairs per wave, one copy of all 64 lanes, and the header in a copy of its own (lane 0): Map<8>::kPairCopies = 2
template <int NW>
__device__ __forceinline__ void issue_pairs(const int32_t *__restrict__ pairs, const int4 *__restrict__ recs, int64_t k, int64_t k1,
                                            int slot, char *smem, int wave, int lane) {
    if constexpr (NW == 8) {
        lane = lane_id_here();
        const int32_t *src = pairs + k * (int64_t)(TRS * SB * 2) + wave * (Map<8>::kWaveRec / 4) + lane * 4;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(smem + Map<8>::ring_slot(0, wave, slot)), 16, 0, 0);
        if (lane == 0)
            __builtin_amdgcn_global_load_lds((gptr_t)(recs + (k + 1 < k1 ? k + 1 : k)), (lptr_t)(smem + Map<8>::header(0, wave, slot)), 16, 0, 0);
        return;
    }
    if (lane <= 32) {
        const int32_t *src = lane < 32 ? pairs + k * (int64_t)(TRS * SB * 2) + wave * (kWaveRec / 4) + lane * 4
                                       : reinterpret_cast<const int32_t *>(recs + (k + 1 < k1 ? k + 1 : k));
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(smem + kOffRing + (wave * kRing + slot) * kSlotBytes), 16, 0, 0);
    }
}

__device__ __forceinline__ void fma_chunk(f32x2 (&acc)[2], float w, const f32x4 &x) {
    const f32x2 ww = {w, w};
    acc[0] = __builtin_elementwise_fma(ww, f32x2{x.x, x.y}, acc[0]);
    acc[1] = __builtin_elementwise_fma(ww, f32x2{x.z, x.w}, acc[1]);
}

// One record (layer) of the piece: 8 row slots x 2 entries for this lane's group.  ISSUE: the four copies of the
// next run's panel go out between the steps (all at once they keep every wave of the workgroup stuck in the issue
// queue for ~2 k clk right after the barrier).  `hn` receives the header of the NEXT record (kept behind this
// record's pairs in the ring slot), read under the last steps.
// 8 waves (NS = 16 steps): the eight steps run twice, once per owned row group; the second pass reads its pairs 512 B further
// into the ring slot (Map::pair_off) and feeds the other half of the accumulators.  The two passes are ONE pipeline: steps 6
// and 7 of the first already fetch the pairs and rows of the second (two waves per SIMD do not hide a drained LDS pipe), the
// header is read under the last two steps of the second, and the eight panel copies go out one per two steps.
template <int NW>
__device__ __forceinline__ void compute_record(const int ISSUE, f32x2 (&acc)[Map<NW>::kSteps][2][2], const uint32_t pa, const uint32_t rowbase, f32x4 &hn,
                                               uint32_t hdr, int next_panel, uint32_t lds0, int pbn, const float *__restrict__ B, int64_t ldb,
                                               int64_t ncols, int fcol0, uint32_t lane_off, int wave) {
    constexpr int NS = Map<NW>::kSteps;
    f32x4 pA, pB, pC, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3;
    lds_read_b128<Map<NW>::pair_off(0)>(pA, pa);
    lds_read_b128<Map<NW>::pair_off(1)>(pB, pa);
    lds_wait1(pA);
    {
        const uint32_t a0 = rowbase + (uint32_t)__float_as_int(pA.x), a1 = rowbase + (uint32_t)__float_as_int(pA.z);
        lds_read_b128<0>(xa0, a0);
        lds_read_b128<256>(xa1, a0);
        lds_read_b128<0>(xa2, a1);
        lds_read_b128<256>(xa3, a1);
    }
    // step S (P = pairs of step S, N = pairs of step S + 1, M = free): the rows of step S and N have landed; the rows
    // of step S + 1 and the pairs of step S + 2 go out BEFORE the packed FMAs of step S (sched_barrier pins that
    // order), so the LDS pipe always holds five reads of this wave.  hdr: where the next record's header is read -- 16 waves: the
    // wave's ring slot as a per-lane value (pa minus the group's offset; the header sits kWaveRec behind it), 8 waves: the header's
    // own address, wave-uniform, so that no per-lane value has to stay live for it
#define PGCN_STRIP_STEP(S, P, N, M, XA0, XA1, XA2, XA3, XB0, XB1, XB2, XB3)              \
    if constexpr ((S) < NS) {                                                              \
        if constexpr ((S) + 1 < NS) {                                                      \
            lds_wait0(XA0, XA1, XA2, XA3, N);                                              \
            const uint32_t a0 = rowbase + (uint32_t)__float_as_int(N.x);                   \
            const uint32_t a1 = rowbase + (uint32_t)__float_as_int(N.z);                   \
            lds_read_b128<0>(XB0, a0);                                                     \
            lds_read_b128<256>(XB1, a0);                                                   \
            lds_read_b128<0>(XB2, a1);                                                     \
            lds_read_b128<256>(XB3, a1);                                                   \
            if constexpr ((S) + 2 < NS) { lds_read_b128<Map<NW>::pair_off(((S) + 2) % NS)>(M, pa); } \
            else { lds_read_b128<(NW == 16 ? Map<NW>::kWaveRec : 0)>(hn, hdr); }           \
        } else {                                                                           \
            lds_wait0(XA0, XA1, XA2, XA3, hn);                                             \
        }                                                                                  \
        if constexpr (((S) & 1) == 0)                                                      \
            issue_panel_if<(S) / 2, NW>(ISSUE, next_panel, lds0, pbn, B, ldb, ncols, fcol0, lane_off, wave); \
        __builtin_amdgcn_sched_barrier(0);                                                 \
        fma_chunk(acc[(S) % NS][0], P.y, XA0);                                             \
        fma_chunk(acc[(S) % NS][1], P.y, XA1);                                             \
        fma_chunk(acc[(S) % NS][0], P.w, XA2);                                             \
        fma_chunk(acc[(S) % NS][1], P.w, XA3);                                             \
        __builtin_amdgcn_sched_barrier(0);                                                 \
    }
    PGCN_STRIP_STEP(0, pA, pB, pC, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3)
    PGCN_STRIP_STEP(1, pB, pC, pA, xb0, xb1, xb2, xb3, xa0, xa1, xa2, xa3)
    PGCN_STRIP_STEP(2, pC, pA, pB, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3)
    PGCN_STRIP_STEP(3, pA, pB, pC, xb0, xb1, xb2, xb3, xa0, xa1, xa2, xa3)
    PGCN_STRIP_STEP(4, pB, pC, pA, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3)
    PGCN_STRIP_STEP(5, pC, pA, pB, xb0, xb1, xb2, xb3, xa0, xa1, xa2, xa3)
    PGCN_STRIP_STEP(6, pA, pB, pC, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3)
    PGCN_STRIP_STEP(7, pB, pC, pA, xb0, xb1, xb2, xb3, xa0, xa1, xa2, xa3)
    PGCN_STRIP_STEP(8, pC, pA, pB, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3)
    PGCN_STRIP_STEP(9, pA, pB, pC, xb0, xb1, xb2, xb3, xa0, xa1, xa2, xa3)
    PGCN_STRIP_STEP(10, pB, pC, pA, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3)
    PGCN_STRIP_STEP(11, pC, pA, pB, xb0, xb1, xb2, xb3, xa0, xa1, xa2, xa3)
    PGCN_STRIP_STEP(12, pA, pB, pC, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3)
    PGCN_STRIP_STEP(13, pB, pC, pA, xb0, xb1, xb2, xb3, xa0, xa1, xa2, xa3)
    PGCN_STRIP_STEP(14, pC, pA, pB, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3)
    PGCN_STRIP_STEP(15, pA, pB, pC, xb0, xb1, xb2, xb3, xa0, xa1, xa2, xa3)
#undef PGCN_STRIP_STEP
}

// work: int4 {tile row, first record, one-past-last record, first slot}
// recs: int4 {panel, flags, next panel, layer}; flags bit 0: the panel is the one of the previous record of the
//       piece; `next panel` (records that start a run of one panel): panel of the piece's NEXT run or -1
// PROBE (measurement aid, PGCN_STRIP_PROBE): 1 = no compute phase, 2 = no panel staging, 4 = phase timers
// NW: waves per workgroup, 16 or 8 (pgcn_strip_map.h); every count below that differs between the two comes from Map<NW>
template <int PROBE, int NW = 16>
__global__ __launch_bounds__(NW * 64, 1) void spmm_strip_kernel(
    const int4 *__restrict__ work, const int4 *__restrict__ recs, const int32_t *__restrict__ pairs,
    const float *__restrict__ B, int64_t ldb, int64_t ncols, int32_t f, float *__restrict__ partial,
    const int32_t *__restrict__ run_if) {
    using M = Map<NW>;
    constexpr int NP = M::kPanelCopies, PC = M::kPairCopies, NS = M::kSteps;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (pgcn_group_off(run_if)) return;    // (pgcn_spmm_strip_if_f32: ahead of every access and of the scheduled blocks below)
    int4 wk = work[blockIdx.x];
    wk.x = __builtin_amdgcn_readfirstlane(wk.x); wk.y = __builtin_amdgcn_readfirstlane(wk.y);   // wave-uniform: scalar control flow
    wk.z = __builtin_amdgcn_readfirstlane(wk.z); wk.w = __builtin_amdgcn_readfirstlane(wk.w);
    const int fcol0 = blockIdx.y * 128;
    const int fw = min(128, f - fcol0);
    int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int s = lane & 15;
    const int gq = (lane >> 4);            // group inside the wave
    int g = M::row_group(wave, 0, gq);     // the row group of the first pass, 0..63 (8 waves: the second pass owns g + 4)
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)smem;
    // panel copies: thread t moves 16 B of row (q * 32 + t / 32), chunk t % 32 (8 waves: q * 16 + t / 32; narrow panels repeat their last chunk)
    const int c4s = min((int)(threadIdx.x & 31), (fw >> 2) - 1);
    const uint32_t lane_off = (uint32_t)(((int64_t)(threadIdx.x >> 5) * ldb + c4s * 4) * 4);

    f32x2 acc[NS][2][2];                   // row slot j of pass p: acc[p * 8 + j]
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j][0][0] = acc[j][0][1] = acc[j][1][0] = acc[j][1][1] = f32x2{0.f, 0.f};
    if (threadIdx.x < 64)   // the all-zero row of both panel buffers
        *reinterpret_cast<float4 *>(smem + (threadIdx.x >> 5) * kPanelBytes + kPadOff + (threadIdx.x & 31) * 16) =
            make_float4(0.f, 0.f, 0.f, 0.f);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // ... has left this wave before the first barrier

    const int k0 = wk.y, k1 = wk.z;
    int4 rc = recs[k0];                    // header of the current record; the later ones arrive with the pairs
    rc.x = __builtin_amdgcn_readfirstlane(rc.x); rc.y = __builtin_amdgcn_readfirstlane(rc.y);
    rc.z = __builtin_amdgcn_readfirstlane(rc.z);
    int pb = 0, pbn = 0;
    if (!(PROBE & 2)) issue_panel<0, NP, NW>(rc.x, lds0, 0, B, ldb, ncols, fcol0, lane_off, wave);
    issue_pairs<NW>(pairs, recs, k0, k1, 0, smem, wave, lane);
    bool have_next = k0 + 1 < k1;          // the pairs of record k + 1 are in flight
    if (have_next) issue_pairs<NW>(pairs, recs, k0 + 1, k1, 1, smem, wave, lane);
    // vmcnt bookkeeping (copies complete in issue order): what this wave issued AFTER the copies it waits for, counted in
    // instructions: NP per panel, PC per ring slot (8 waves: pairs, then the header, both awaited together)
    int after_panel = have_next ? 2 * PC : PC;   // ... after the latest panel copies (saturates at two ring slots)
    bool issued1 = false, issued2 = false; // panel copies went out during the previous record / the one before
    int slot = 0, in_run = 0;
    // 16 waves: the pair and row addresses are formed per record; 8 waves: two registers moved in place (ring slot, panel buffer)
    uint32_t pa8 = 0, rowbase8 = 0;
    if constexpr (NW == 8) { pa8 = M::pair_base(lds0, wave, 0, gq); rowbase8 = M::row_base(lds0, 0, s); }
    long long t_vm = 0, t_bar = 0, t_cmp = 0, t0 = 0, t1;
    for (int k = k0; k < k1; ++k) {
        if constexpr (PROBE & 4) t0 = __builtin_readcyclecounter();
        // issue order of an iteration: [pairs k + 2] [panel of the next run, during the compute phase]
        int nafter = (issued2 ? NP : 0) + (issued1 ? NP : 0) + (k + 1 < k1 ? PC : 0);
        if (k + 2 < k1) {
            int s2 = slot + 2; s2 = s2 >= kRing ? s2 - kRing : s2;
            issue_pairs<NW>(pairs, recs, k + 2, k1, s2, smem, wave, lane);
            after_panel = after_panel < 2 * PC ? after_panel + PC : 2 * PC;
            nafter += PC;
        }
        wait_vm_dyn<NW>(nafter);               // the pairs of record k have landed in this wave's ring
        if constexpr (PROBE & 4) { t1 = __builtin_readcyclecounter(); t_vm += t1 - t0; t0 = t1; }
        // The issue arbiter serves the waves of a SIMD oldest first: without help wave 0 finishes a run 1.5x sooner
        // than wave 15 and idles at the next barrier while the LDS pipe starves on the few waves left.  A wave that
        // is ahead lowers its own priority (3, 2, 1, 0 for the first, second, ... record after a barrier).
        if (!(rc.y & 1)) in_run = 0;
        switch (in_run) {
            case 0: __builtin_amdgcn_s_setprio(3); break;
            case 1: __builtin_amdgcn_s_setprio(2); break;
            case 2: __builtin_amdgcn_s_setprio(1); break;
            default: __builtin_amdgcn_s_setprio(0); break;
        }
        ++in_run;
        bool cur_issued = false;
        if (!(rc.y & 1)) {                 // this record starts a run of a new panel
            wait_vm_dyn<NW>(after_panel);      // this wave's copies of the panel have landed
            __builtin_amdgcn_s_barrier();  // ... everybody's have, and nobody reads the other buffer any more
            if constexpr (NW == 8) add_uniform(rowbase8, (pbn - pb) * kPanelBytes);
            pb = pbn;
            if (rc.z >= 0 && !(PROBE & 2)) {
                pbn = pb ^ 1;
                cur_issued = true;         // (the copies go out inside compute_record)
                after_panel = 0;
            }
        }
        if constexpr (PROBE & 4) { t1 = __builtin_readcyclecounter(); t_bar += t1 - t0; t0 = t1; }
        const uint32_t pa = NW == 16 ? M::pair_base(lds0, wave, slot, gq) : pa8;
        const uint32_t rowbase = NW == 16 ? M::row_base(lds0, pb, s) : rowbase8;
        const uint32_t hdr = NW == 16 ? pa - gq * (RW * SB * 8) : M::header(lds0, wave, slot);
        f32x4 hn;
        if constexpr (!(PROBE & 1)) {
            compute_record<NW>(cur_issued ? 1 : 0, acc, pa, rowbase, hn, hdr, rc.z, lds0, pbn, B, ldb, ncols, fcol0, lane_off, wave);
        } else {
            if (cur_issued) issue_panel<0, NP, NW>(rc.z, lds0, pbn, B, ldb, ncols, fcol0, lane_off, wave);
            lds_read_b128<(NW == 16 ? M::kWaveRec : 0)>(hn, hdr);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(hn));
        }
        rc.x = __builtin_amdgcn_readfirstlane(__float_as_int(hn.x));
        rc.y = __builtin_amdgcn_readfirstlane(__float_as_int(hn.y));
        rc.z = __builtin_amdgcn_readfirstlane(__float_as_int(hn.z));
        if constexpr (PROBE & 4) { t1 = __builtin_readcyclecounter(); t_cmp += t1 - t0; }
        issued2 = issued1;
        issued1 = cur_issued;
        if constexpr (NW == 8) add_uniform(pa8, slot + 1 >= kRing ? -(kRing - 1) * M::kSlotBytes : M::kSlotBytes);
        slot = slot + 1 >= kRing ? 0 : slot + 1;
    }
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (NW == 8) {               // (see lane_id_here)
        lane = lane_id_here();
        s = lane & 15;
        g = M::row_group(wave, 0, lane >> 4);
    }
    if constexpr (PROBE & 4) {             // timer ticks per record of the phases, one row of the slot block per wave
        if (lane == 0) {
            float *o = partial + ((int64_t)wk.w + wave) * f + fcol0;
            const float nr = (float)(k1 - k0);
            o[0] = (float)t_vm / nr; o[1] = 0.f; o[2] = (float)t_bar / nr; o[3] = (float)t_cmp / nr;
        }
        return;
    }
    if (fw >= 128) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {     // accumulator j: row slot j % 8 of row group g + 4 * (j / 8)
            float *o = partial + ((int64_t)wk.w + (j % RW) * NG + (j / RW) * 4 + g) * f + fcol0 + s * 4;
            *reinterpret_cast<float4 *>(o) = make_float4(acc[j][0][0].x, acc[j][0][0].y, acc[j][0][1].x, acc[j][0][1].y);
            *reinterpret_cast<float4 *>(o + 64) = make_float4(acc[j][1][0].x, acc[j][1][0].y, acc[j][1][1].x, acc[j][1][1].y);
        }
    } else {
#pragma unroll
        for (int j = 0; j < NS; ++j) {     // accumulator j: row slot j % 8 of row group g + 4 * (j / 8)
            float *o = partial + ((int64_t)wk.w + (j % RW) * NG + (j / RW) * 4 + g) * f + fcol0 + s * 4;
            if (s * 4 < fw) *reinterpret_cast<float4 *>(o) = make_float4(acc[j][0][0].x, acc[j][0][0].y, acc[j][0][1].x, acc[j][0][1].y);
            if (64 + s * 4 < fw)
                *reinterpret_cast<float4 *>(o + 64) = make_float4(acc[j][1][0].x, acc[j][1][0].y, acc[j][1][1].x, acc[j][1][1].y);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Value-free records (structures with no values: a 0/1 pattern P, or diag(r) P diag(c)).  A record keeps only the 4-byte
// offset slots: 1 024 x 4 B = 4 KB, same row order, unused slots point at the zero row.  c_j reaches the FMAs through the
// staged panel: every thread multiplies the four 16-byte chunks IT copied by the c of their rows after its own copies have
// landed and BEFORE the one barrier of the panel change (nobody else touches those bytes, so no second barrier), i.e. once per
// staged row instead of once per entry, and the compute phase is the stored kernel's with weight 1 (an all-ones structure
// gives the stored kernel's sums bit for bit).  r_i is applied at the partial-row write; the fix-up is unchanged.
constexpr int kWaveRecVF = TRS * SB * 4 / (kThreads / 64);   // 256 B: the offsets of one wave's four groups
constexpr int kSlotBytesVF = kWaveRecVF + 16;
constexpr int kGroupVF = RW * SB * 4;                          // 64 B per group and record
constexpr int kSmemVF = kOffRing + (kThreads / 64) * kRing * kSlotBytesVF;

__device__ __forceinline__ void issue_offs(const int32_t *__restrict__ offs, const int4 *__restrict__ recs, int64_t k, int64_t k1,
                                           int slot, char *smem, int wave, int lane) {
    if (lane <= 16) {
        const int32_t *src = lane < 16 ? offs + k * (int64_t)(TRS * SB) + wave * (kWaveRecVF / 4) + lane * 4
                                       : reinterpret_cast<const int32_t *>(recs + (k + 1 < k1 ? k + 1 : k));
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(smem + kOffRing + (wave * kRing + slot) * kSlotBytesVF), 16, 0, 0);
    }
}

__device__ __forceinline__ void lds_wait0_q(f32x4 &a, f32x4 &b, f32x4 &c, f32x4 &d, f32x4 &q, f32x4 &h) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(q), "+v"(h));
}

// One value-free record: the offsets of row slots 2m and 2m + 1 arrive in one ds_read_b128 (Q_m); the rows of slot J + 1 and
// the offsets two slots ahead go out before the FMAs of slot J, as in compute_record.
__device__ __forceinline__ void compute_record_vf(const int ISSUE, f32x2 (&acc)[RW][2][2], const uint32_t pa, const uint32_t rowbase,
                                                  f32x4 &hn, uint32_t gq64, int next_panel, uint32_t lds0, int pbn,
                                                  const float *__restrict__ B, int64_t ldb, int64_t ncols, int fcol0, uint32_t lane_off,
                                                  int wave) {
    f32x4 qa, qb, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3;
    qb = f32x4{0.f, 0.f, 0.f, 0.f};
    lds_read_b128<0>(qa, pa);
    lds_wait1(qa);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(qa));
    {
        const uint32_t a0 = rowbase + (uint32_t)__float_as_int(qa.x), a1 = rowbase + (uint32_t)__float_as_int(qa.y);
        lds_read_b128<0>(xa0, a0);
        lds_read_b128<256>(xa1, a0);
        lds_read_b128<0>(xa2, a1);
        lds_read_b128<256>(xa3, a1);
    }
    // step J: X = rows of slot J (landed at the wait), NQ = the register holding slot J + 1's offsets (.xy for odd J + 1, .zw for
    // even), FQ = the register Q_(J/2+1) is read into (even J).  The last even step reads the next record's header instead.
#define PGCN_STRIP_VF_STEP(J, NQ, FQ, XA0, XA1, XA2, XA3, XB0, XB1, XB2, XB3)                                      \
    {                                                                                                             \
        lds_wait0_q(XA0, XA1, XA2, XA3, NQ, hn);                                                                  \
        if ((J) + 1 < RW) {                                                                                       \
            const uint32_t a0 = rowbase + (uint32_t)__float_as_int(((J) & 1) ? NQ.x : NQ.z);                      \
            const uint32_t a1 = rowbase + (uint32_t)__float_as_int(((J) & 1) ? NQ.y : NQ.w);                      \
            lds_read_b128<0>(XB0, a0);                                                                            \
            lds_read_b128<256>(XB1, a0);                                                                          \
            lds_read_b128<0>(XB2, a1);                                                                            \
            lds_read_b128<256>(XB3, a1);                                                                          \
            if (((J) & 1) == 0) {                                                                                 \
                if ((J) + 2 < RW) { lds_read_b128<(((J) / 2 + 1) * 16)>(FQ, pa); }                                \
                else { lds_read_b128<kWaveRecVF>(hn, pa - gq64); }                                                \
            }                                                                                                     \
        }                                                                                                         \
        if (((J) & 1) == 0)                                                                                       \
            issue_panel_if<(J) / 2>(ISSUE, next_panel, lds0, pbn, B, ldb, ncols, fcol0, lane_off, wave);         \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        fma_chunk(acc[(J)][0], 1.f, XA0);                                                                         \
        fma_chunk(acc[(J)][1], 1.f, XA1);                                                                         \
        fma_chunk(acc[(J)][0], 1.f, XA2);                                                                         \
        fma_chunk(acc[(J)][1], 1.f, XA3);                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    }
    PGCN_STRIP_VF_STEP(0, qa, qb, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3)
    PGCN_STRIP_VF_STEP(1, qb, qa, xb0, xb1, xb2, xb3, xa0, xa1, xa2, xa3)
    PGCN_STRIP_VF_STEP(2, qb, qa, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3)
    PGCN_STRIP_VF_STEP(3, qa, qb, xb0, xb1, xb2, xb3, xa0, xa1, xa2, xa3)
    PGCN_STRIP_VF_STEP(4, qa, qb, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3)
    PGCN_STRIP_VF_STEP(5, qb, qa, xb0, xb1, xb2, xb3, xa0, xa1, xa2, xa3)
    PGCN_STRIP_VF_STEP(6, qb, qa, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3)
    PGCN_STRIP_VF_STEP(7, qa, qb, xb0, xb1, xb2, xb3, xa0, xa1, xa2, xa3)
#undef PGCN_STRIP_VF_STEP
}

// The thread's four chunks of the panel in buffer `pb` (copied by issue_panel*: row q * 32 + t / 32) times c of their rows.
__device__ __forceinline__ void scale_own_panel(char *smem, int pb, int panel, const float *__restrict__ col_scale, int64_t ncols) {
    int64_t col0 = (int64_t)panel * TC;
    col0 = col0 + TC <= ncols ? col0 : ncols - TC;
    float s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = col_scale[col0 + q * 32 + (threadIdx.x >> 5)];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float4 *p = reinterpret_cast<float4 *>(smem + pb * kPanelBytes + (q * kThreads + threadIdx.x) * 16);
        float4 x = *p;
        x.x *= s[q]; x.y *= s[q]; x.z *= s[q]; x.w *= s[q];
        *p = x;
    }
}

// work / recs: as spmm_strip_kernel; offs: int32 [nrec][1024] value-free records; col_scale (NULL: ones) [ncols];
// row_scale (NULL: ones): r of the matrix rows, readable at rows 512 * tile row + 0 .. 511 of every piece.
__global__ __launch_bounds__(kThreads, 1) void spmm_strip_vf_kernel(
    const int4 *__restrict__ work, const int4 *__restrict__ recs, const int32_t *__restrict__ offs,
    const float *__restrict__ row_scale, const float *__restrict__ col_scale,
    const float *__restrict__ B, int64_t ldb, int64_t ncols, int32_t f, float *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int4 wk = work[blockIdx.x];
    wk.x = __builtin_amdgcn_readfirstlane(wk.x); wk.y = __builtin_amdgcn_readfirstlane(wk.y);
    wk.z = __builtin_amdgcn_readfirstlane(wk.z); wk.w = __builtin_amdgcn_readfirstlane(wk.w);
    const int fcol0 = blockIdx.y * 128;
    const int fw = min(128, f - fcol0);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s = lane & 15;
    const int gq = (lane >> 4);
    const int g = wave * 4 + gq;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)smem;
    const int c4s = min((int)(threadIdx.x & 31), (fw >> 2) - 1);
    const uint32_t lane_off = (uint32_t)(((int64_t)(threadIdx.x >> 5) * ldb + c4s * 4) * 4);

    f32x2 acc[RW][2][2];
#pragma unroll
    for (int j = 0; j < RW; ++j) acc[j][0][0] = acc[j][0][1] = acc[j][1][0] = acc[j][1][1] = f32x2{0.f, 0.f};
    if (threadIdx.x < 64)
        *reinterpret_cast<float4 *>(smem + (threadIdx.x >> 5) * kPanelBytes + kPadOff + (threadIdx.x & 31) * 16) =
            make_float4(0.f, 0.f, 0.f, 0.f);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    const int k0 = wk.y, k1 = wk.z;
    int4 rc = recs[k0];
    rc.x = __builtin_amdgcn_readfirstlane(rc.x); rc.y = __builtin_amdgcn_readfirstlane(rc.y);
    rc.z = __builtin_amdgcn_readfirstlane(rc.z);
    int pb = 0, pbn = 0;
    issue_panel<0, 4>(rc.x, lds0, 0, B, ldb, ncols, fcol0, lane_off, wave);
    issue_offs(offs, recs, k0, k1, 0, smem, wave, lane);
    bool have_next = k0 + 1 < k1;
    if (have_next) issue_offs(offs, recs, k0 + 1, k1, 1, smem, wave, lane);
    int after_panel = have_next ? 2 : 1;
    bool issued1 = false, issued2 = false;
    int slot = 0, in_run = 0;
    for (int k = k0; k < k1; ++k) {
        int nafter = (issued2 ? 4 : 0) + (issued1 ? 4 : 0) + (k + 1 < k1 ? 1 : 0);
        if (k + 2 < k1) {
            int s2 = slot + 2; s2 = s2 >= kRing ? s2 - kRing : s2;
            issue_offs(offs, recs, k + 2, k1, s2, smem, wave, lane);
            after_panel = after_panel < 2 ? after_panel + 1 : 2;
            ++nafter;
        }
        wait_vm_dyn<16>(nafter);
        if (!(rc.y & 1)) in_run = 0;
        switch (in_run) {
            case 0: __builtin_amdgcn_s_setprio(3); break;
            case 1: __builtin_amdgcn_s_setprio(2); break;
            case 2: __builtin_amdgcn_s_setprio(1); break;
            default: __builtin_amdgcn_s_setprio(0); break;
        }
        ++in_run;
        bool cur_issued = false;
        if (!(rc.y & 1)) {
            wait_vm_dyn<16>(after_panel);  // this thread's copies of the panel have landed ...
            if (col_scale) {               // ... it scales exactly those bytes, then the one barrier publishes them
                scale_own_panel(smem, pbn, rc.x, col_scale, ncols);
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
            pb = pbn;
            if (rc.z >= 0) {
                pbn = pb ^ 1;
                cur_issued = true;
                after_panel = 0;
            }
        }
        const uint32_t pa = lds0 + kOffRing + (wave * kRing + slot) * kSlotBytesVF + gq * kGroupVF;
        const uint32_t rowbase = lds0 + pb * kPanelBytes + s * 16;
        f32x4 hn = f32x4{0.f, 0.f, 0.f, 0.f};
        compute_record_vf(cur_issued ? 1 : 0, acc, pa, rowbase, hn, gq * kGroupVF, rc.z, lds0, pbn, B, ldb, ncols, fcol0, lane_off, wave);
        rc.x = __builtin_amdgcn_readfirstlane(__float_as_int(hn.x));
        rc.y = __builtin_amdgcn_readfirstlane(__float_as_int(hn.y));
        rc.z = __builtin_amdgcn_readfirstlane(__float_as_int(hn.z));
        issued2 = issued1;
        issued1 = cur_issued;
        slot = slot + 1 >= kRing ? 0 : slot + 1;
    }
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < RW; ++j) {
        const float r = row_scale ? row_scale[(int64_t)wk.x * TRS + j * NG + g] : 1.f;
        float *o = partial + ((int64_t)wk.w + j * NG + g) * f + fcol0 + s * 4;
        const float4 lo = make_float4(acc[j][0][0].x * r, acc[j][0][0].y * r, acc[j][0][1].x * r, acc[j][0][1].y * r);
        const float4 hi = make_float4(acc[j][1][0].x * r, acc[j][1][0].y * r, acc[j][1][1].x * r, acc[j][1][1].y * r);
        if (s * 4 < fw) *reinterpret_cast<float4 *>(o) = lo;
        if (64 + s * 4 < fw) *reinterpret_cast<float4 *>(o + 64) = hi;
    }
}

// Any width / alignment, value-free records: operands read straight from global memory (correctness path).
__global__ __launch_bounds__(kThreads, 1) void spmm_strip_vf_generic_kernel(
    const int4 *__restrict__ work, const int4 *__restrict__ recs, const int32_t *__restrict__ offs,
    const float *__restrict__ row_scale, const float *__restrict__ col_scale,
    const float *__restrict__ B, int64_t ldb, int64_t ncols, int32_t f, float *__restrict__ partial) {
    const int4 wk = work[blockIdx.x];
    const int sub = threadIdx.x & 31;
    const int g32 = threadIdx.x >> 5;
    const int fcol = blockIdx.y * 32 + sub;
    const bool fact = fcol < f;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k = wk.y; k < wk.z; ++k) {
        int64_t col0 = (int64_t)recs[k].x * TC;
        col0 = col0 + TC <= ncols ? col0 : ncols - TC;
        const int32_t *pr = offs + (int64_t)k * TRS * SB;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = i * 32 + g32;
            const int32_t *pp = pr + ((row % NG) * RW + row / NG) * SB;
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int32_t off = pp[u];
                if (off != kPadOff && fact) {
                    const int64_t c = col0 + (off >> 9);
                    const float x = col_scale ? B[c * ldb + fcol] * col_scale[c] : B[c * ldb + fcol];
                    acc[i] = fmaf(1.f, x, acc[i]);
                }
            }
        }
    }
    if (fact) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = i * 32 + g32;
            const float r = row_scale ? row_scale[(int64_t)wk.x * TRS + row] : 1.f;
            partial[((int64_t)wk.w + row) * f + fcol] = acc[i] * r;
        }
    }
}

// Any width / alignment: same records, operands read straight from global memory, one feature per
// lane (blockIdx.y walks the features 32 at a time).  Correctness path, not a fast path.
__global__ __launch_bounds__(kThreads, 1) void spmm_strip_generic_kernel(
    const int4 *__restrict__ work, const int4 *__restrict__ recs, const int32_t *__restrict__ pairs,
    const float *__restrict__ B, int64_t ldb, int64_t ncols, int32_t f, float *__restrict__ partial,
    const int32_t *__restrict__ run_if) {
    if (pgcn_group_off(run_if)) return;
    const int4 wk = work[blockIdx.x];
    const int sub = threadIdx.x & 31;
    const int g32 = threadIdx.x >> 5;      // 32 groups of 32 lanes, 16 rows each: row = i * 32 + g32
    const int fcol = blockIdx.y * 32 + sub;
    const bool fact = fcol < f;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k = wk.y; k < wk.z; ++k) {
        int64_t col0 = (int64_t)recs[k].x * TC;
        col0 = col0 + TC <= ncols ? col0 : ncols - TC;   // the last panel is the window [ncols - 128, ncols)
        const int32_t *pr = pairs + (int64_t)k * TRS * SB * 2;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = i * 32 + g32;
            const int32_t *pp = pr + (((row % NG) * RW + row / NG) * SB) * 2;
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int32_t off = pp[u * 2];
                const float w = __int_as_float(pp[u * 2 + 1]);
                if (off != kPadOff && fact) acc[i] = fmaf(w, B[(col0 + (off >> 9)) * ldb + fcol], acc[i]);
            }
        }
    }
    if (fact) {
#pragma unroll
        for (int i = 0; i < 16; ++i) partial[((int64_t)wk.w + i * 32 + g32) * f + fcol] = acc[i];
    }
}

}  // namespace

// The stored-record entry points: NW waves per workgroup; `who` names the plain entry point in the messages.  run_if == NULL: the plain
// call; otherwise every workgroup returns at once when the device word is 0.
template <int NW>
static int strip_launch(const char *who, const int32_t *work, int64_t nwork, const int32_t *recs, const int32_t *pairs,
                        const float *B, int64_t ldb, int64_t ncols, int32_t f, float *partial_ws,
                        int64_t partial_ws_elems, int64_t nslots_total, const int32_t *run_if, pgcn_stream_t stream) {
    if (nwork < 0 || f <= 0 || ldb < f || ncols < TC) return pgcn_set_error2(PGCN_EINVAL, who, "bad sizes (a panel is 128 rows of B)");
    if (ldb > kMaxLdb)
        return pgcn_set_error2(PGCN_EINVAL, who, "leading dimension ldb too large for the 32-bit lane offsets of the panel copies (at most 34636829 floats)");
    if (nwork == 0) return PGCN_OK;
    if (!work || !recs || !pairs || !B || !partial_ws)
        return pgcn_set_error2(PGCN_EINVAL, who, "null pointer");
    if (partial_ws_elems < nslots_total * (int64_t)f)
        return pgcn_set_error2(PGCN_ENOMEM, who, "partial work-space too small");
    if (nwork > 0x7fffffffLL) return pgcn_set_error2(PGCN_EINVAL, who, "work list too long");
    if ((uintptr_t)pairs % 16 || (uintptr_t)recs % 16 || (uintptr_t)work % 16)
        return pgcn_set_error2(PGCN_EINVAL, who, "work / recs / pairs must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int4 *w4 = reinterpret_cast<const int4 *>(work);
    const int4 *r4 = reinterpret_cast<const int4 *>(recs);
    const bool vec = f % 4 == 0 && ldb % 4 == 0 && (uintptr_t)B % 16 == 0 && (uintptr_t)partial_ws % 16 == 0;
    if (vec) {
        constexpr int smem = Map<NW>::kSmem, threads = Map<NW>::kThreads;
        static PgcnPerDeviceOnce once;
        if (int rc = once.run([&]() -> int {
                PGCN_HIP_CHECK(hipFuncSetAttribute((const void *)spmm_strip_kernel<0, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
#ifdef PGCN_EXPERIMENTS
                PGCN_HIP_CHECK(hipFuncSetAttribute((const void *)spmm_strip_kernel<1, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
                PGCN_HIP_CHECK(hipFuncSetAttribute((const void *)spmm_strip_kernel<2, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
                PGCN_HIP_CHECK(hipFuncSetAttribute((const void *)spmm_strip_kernel<4, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
#endif
                return PGCN_OK;
            }))
            return rc;
        const dim3 grid((unsigned)nwork, (unsigned)((f + 127) / 128));
#ifdef PGCN_EXPERIMENTS
        // measurement build only (tools/ab_build.sh exp -DPGCN_EXPERIMENTS): PGCN_STRIP_PROBE = 1 no compute phase,
        // 2 no panel staging, 4 phase timers instead of results
        static const int probe = getenv("PGCN_STRIP_PROBE") ? atoi(getenv("PGCN_STRIP_PROBE")) : 0;
        if (probe == 1) hipLaunchKernelGGL((spmm_strip_kernel<1, NW>), grid, dim3(threads), smem, s, w4, r4, pairs, B, ldb, ncols, f, partial_ws, run_if);
        else if (probe == 2) hipLaunchKernelGGL((spmm_strip_kernel<2, NW>), grid, dim3(threads), smem, s, w4, r4, pairs, B, ldb, ncols, f, partial_ws, run_if);
        else if (probe == 4) hipLaunchKernelGGL((spmm_strip_kernel<4, NW>), grid, dim3(threads), smem, s, w4, r4, pairs, B, ldb, ncols, f, partial_ws, run_if);
        else
#endif
        hipLaunchKernelGGL((spmm_strip_kernel<0, NW>), grid, dim3(threads), smem, s, w4, r4, pairs, B, ldb, ncols, f, partial_ws, run_if);
    } else {
        hipLaunchKernelGGL(spmm_strip_generic_kernel, dim3((unsigned)nwork, (unsigned)((f + 31) / 32)), dim3(kThreads), 0, s,
                           w4, r4, pairs, B, ldb, ncols, f, partial_ws, run_if);
    }
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_spmm_strip_if_f32(const int32_t *work, int64_t nwork, const int32_t *recs, const int32_t *pairs,
                                       const float *B, int64_t ldb, int64_t ncols, int32_t f, float *partial_ws,
                                       int64_t partial_ws_elems, int64_t nslots_total, const int32_t *run_if,
                                       pgcn_stream_t stream) {
    return strip_launch<16>("pgcn_spmm_strip_f32", work, nwork, recs, pairs, B, ldb, ncols, f, partial_ws, partial_ws_elems, nslots_total, run_if, stream);
}

extern "C" int pgcn_spmm_strip_f32(const int32_t *work, int64_t nwork, const int32_t *recs, const int32_t *pairs,
                                    const float *B, int64_t ldb, int64_t ncols, int32_t f, float *partial_ws,
                                    int64_t partial_ws_elems, int64_t nslots_total, pgcn_stream_t stream) {
    return pgcn_spmm_strip_if_f32(work, nwork, recs, pairs, B, ldb, ncols, f, partial_ws, partial_ws_elems, nslots_total, nullptr, stream);
}

// The 8-wave form: the same arguments, refusals and bits; for launch groups whose gather part runs beside the strips (tuning.strip_waves).
extern "C" int pgcn_spmm_strip_w8_if_f32(const int32_t *work, int64_t nwork, const int32_t *recs, const int32_t *pairs,
                                          const float *B, int64_t ldb, int64_t ncols, int32_t f, float *partial_ws,
                                          int64_t partial_ws_elems, int64_t nslots_total, const int32_t *run_if,
                                          pgcn_stream_t stream) {
    return strip_launch<8>("pgcn_spmm_strip_w8_f32", work, nwork, recs, pairs, B, ldb, ncols, f, partial_ws, partial_ws_elems, nslots_total, run_if, stream);
}

extern "C" int pgcn_spmm_strip_w8_f32(const int32_t *work, int64_t nwork, const int32_t *recs, const int32_t *pairs,
                                       const float *B, int64_t ldb, int64_t ncols, int32_t f, float *partial_ws,
                                       int64_t partial_ws_elems, int64_t nslots_total, pgcn_stream_t stream) {
    return pgcn_spmm_strip_w8_if_f32(work, nwork, recs, pairs, B, ldb, ncols, f, partial_ws, partial_ws_elems, nslots_total, nullptr, stream);
}

extern "C" int pgcn_spmm_strip_vf_f32(const int32_t *work, int64_t nwork, const int32_t *recs, const int32_t *offs,
                                       const float *row_scale, const float *col_scale, const float *B, int64_t ldb, int64_t ncols,
                                       int32_t f, float *partial_ws, int64_t partial_ws_elems, int64_t nslots_total,
                                       pgcn_stream_t stream) {
    if (nwork < 0 || f <= 0 || ldb < f || ncols < TC) return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_strip_vf_f32: bad sizes (a panel is 128 rows of B)");
    if (ldb > kMaxLdb)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_strip_vf_f32: leading dimension ldb too large for the 32-bit lane offsets of the panel copies (at most 34636829 floats)");
    if (nwork == 0) return PGCN_OK;
    if (!work || !recs || !offs || !B || !partial_ws)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_strip_vf_f32: null pointer");
    if (partial_ws_elems < nslots_total * (int64_t)f)
        return pgcn_set_error(PGCN_ENOMEM, "pgcn_spmm_strip_vf_f32: partial work-space too small");
    if (nwork > 0x7fffffffLL) return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_strip_vf_f32: work list too long");
    if ((uintptr_t)offs % 16 || (uintptr_t)recs % 16 || (uintptr_t)work % 16)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_spmm_strip_vf_f32: work / recs / offs must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int4 *w4 = reinterpret_cast<const int4 *>(work);
    const int4 *r4 = reinterpret_cast<const int4 *>(recs);
    const bool vec = f % 4 == 0 && ldb % 4 == 0 && (uintptr_t)B % 16 == 0 && (uintptr_t)partial_ws % 16 == 0;
    if (vec) {
        static PgcnPerDeviceOnce once;
        if (int rc = once.run([&]() -> int {
                PGCN_HIP_CHECK(hipFuncSetAttribute((const void *)spmm_strip_vf_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSmemVF));
                return PGCN_OK;
            }))
            return rc;
        hipLaunchKernelGGL(spmm_strip_vf_kernel, dim3((unsigned)nwork, (unsigned)((f + 127) / 128)), dim3(kThreads), kSmemVF, s,
                           w4, r4, offs, row_scale, col_scale, B, ldb, ncols, f, partial_ws);
    } else {
        hipLaunchKernelGGL(spmm_strip_vf_generic_kernel, dim3((unsigned)nwork, (unsigned)((f + 31) / 32)), dim3(kThreads), 0, s,
                           w4, r4, offs, row_scale, col_scale, B, ldb, ncols, f, partial_ws);
    }
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}
