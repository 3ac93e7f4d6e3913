// pgcn_strip_map.h -- the LDS map of spmm_strip_kernel<PROBE, NW> (pgcn_spmm_strip.hip) as plain functions.
//
// The kernel's LDS traffic is inline asm with hand-counted waits, so every address it forms comes from here and a host
// build can evaluate the same arithmetic (tests/native/pgcn_strip_map_host.cpp: every byte of a wave's pairs is read once
// by the right lane group, the panel copies tile a panel buffer exactly, everything fits the CU's 160 KB).
//
// NW = waves per workgroup: 16 (1 024 threads, a strip workgroup has the CU to itself) or 8 (512 threads on the SAME
// records: wave W takes what waves 2 W and 2 W + 1 of the 16 take, in two PASSES over its ring slot, so that gather waves
// fit beside it).  A record is 64 row groups x 128 B (8 row slots x 2 pairs x 8 B); local row = row slot * 64 + group.
#ifndef PGCN_STRIP_MAP_H
#define PGCN_STRIP_MAP_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PGCN_MAP_FN __host__ __device__ constexpr
#else
#define PGCN_MAP_FN constexpr
#endif

namespace pgcn_strip_map {

constexpr int kRows = 512;                          // rows of a strip tile
constexpr int kCols = 128;                          // rows of B in a staged panel
constexpr int kGroups = 64;                         // row groups of a record (16 lanes each)
constexpr int kRowSlots = kRows / kGroups;          // 8
constexpr int kGroupBytes = kRowSlots * 2 * 8;      // 128 B of pairs per group and record
constexpr int kRecBytes = kGroups * kGroupBytes;    // 8 KB
constexpr int kPanelBytes = (kCols + 1) * 512;      // 128 rows x 128 fp32 + the all-zero row
constexpr int kPadOff = kCols * 512;                // what an unused pair slot points at
constexpr int kRing = 3;                            // ring slots per wave (record k, k + 1, k + 2)
constexpr int kOffRing = 2 * kPanelBytes;           // two panel buffers, then the rings
constexpr int kLdsBytes = 160 * 1024;               // LDS of one CU

template <int NW>
struct Map {
    static_assert(NW == 16 || NW == 8, "waves per workgroup");
    static constexpr int kThreads = NW * 64;
    static constexpr int kPasses = 16 / NW;                     // row groups per 16-lane group of a wave
    static constexpr int kSteps = kRowSlots * kPasses;          // compute steps (= accumulator row slots) per record
    static constexpr int kWaveRec = kRecBytes / NW;             // the pairs of one wave: 512 B | 1 KB
    static constexpr int kSlotBytes = kWaveRec + 16;            // ... followed by the NEXT record's 16-byte header
    static constexpr int kPairCopies = kWaveRec / 1024 + 1;     // asynchronous copies per wave and ring slot: 16 waves bring
                                                                // pairs (lanes 0-31) and header (lane 32) in one, 8 waves
                                                                // need all 64 lanes for the pairs and one more for the header
    static constexpr int kPanelCopies = kCols * 512 / 16 / kThreads;   // 16-byte copies per thread and panel: 4 | 8
    static constexpr int kPanelRowsPerCopy = kThreads / 32;     // rows of B that one copy of the whole workgroup moves
    static constexpr int kSmem = kOffRing + NW * kRing * kSlotBytes;

    // LDS addresses; lds0 = where the workgroup's LDS starts (0 on the host)
    static PGCN_MAP_FN uint32_t ring_slot(uint32_t lds0, int wave, int slot) { return lds0 + kOffRing + (wave * kRing + slot) * kSlotBytes; }
    static PGCN_MAP_FN uint32_t header(uint32_t lds0, int wave, int slot) { return ring_slot(lds0, wave, slot) + kWaveRec; }
    // `pa` of lane group gq (0..3): its pairs of pass 0, row slot 0
    static PGCN_MAP_FN uint32_t pair_base(uint32_t lds0, int wave, int slot, int gq) { return ring_slot(lds0, wave, slot) + gq * kGroupBytes; }
    // immediate offset from `pa` of the 16 B of pairs that step S consumes (pass S / 8, row slot S % 8)
    static PGCN_MAP_FN int pair_off(int step) { return (step / kRowSlots) * 4 * kGroupBytes + (step % kRowSlots) * 16; }
    // the record's row group that lane group gq of `wave` owns in `pass`: wave W of 8 = waves 2 W (pass 0), 2 W + 1 (pass 1) of 16
    static PGCN_MAP_FN int row_group(int wave, int pass, int gq) { return (wave * kPasses + pass) * 4 + gq; }
    static PGCN_MAP_FN int local_row(int wave, int step, int gq) { return (step % kRowSlots) * kGroups + row_group(wave, step / kRowSlots, gq); }
    // rows of the staged panel: lane s of a group reads chunks s and s + 16 (offset 256) of the row a pair points at
    static PGCN_MAP_FN uint32_t row_base(uint32_t lds0, int pb, int s) { return lds0 + pb * kPanelBytes + s * 16; }
    // copy q of a panel: the wave-uniform LDS destination (lane l lands 16 l bytes behind it) and its first row of the panel
    static PGCN_MAP_FN uint32_t panel_dst(uint32_t lds0, int pb, int q, int wave) { return lds0 + pb * kPanelBytes + (q * kThreads + wave * 64) * 16; }
    static PGCN_MAP_FN int panel_src_row(int q) { return q * kPanelRowsPerCopy; }
};

static_assert(Map<16>::kSmem <= kLdsBytes && Map<8>::kSmem <= kLdsBytes, "LDS budget of one CU");
static_assert(Map<16>::kPanelCopies == 4 && Map<8>::kPanelCopies == 8 && Map<16>::kPairCopies == 1 && Map<8>::kPairCopies == 2, "copy counts");

}  // namespace pgcn_strip_map
#endif
