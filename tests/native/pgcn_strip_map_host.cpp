// Host check of csrc/pgcn_strip_map.h, the LDS map of spmm_strip_kernel<PROBE, NW> (tests/test_strip_w8.py builds and runs it).
// The kernel's LDS traffic is inline asm with hand-counted waits; every address it forms comes from these functions, so the
// arithmetic is walked here, lane by lane, for both workgroup shapes (16 and 8 waves):
//   1. every byte of a wave's pairs in a ring slot is read exactly once, by the lane group and in the step that own its row, and
//      the 8-wave rows are those of waves 2 W and 2 W + 1 of the 16-wave kernel; the copies fill the slot, the header behind it;
//   2. the panel copies tile a panel buffer exactly, row and chunk where the row reads expect them, the zero row untouched;
//   3. a group's row reads cover a 512-byte row once; everything is 16-byte aligned, disjoint and within the 160 KB of a CU,
//      and the 8-wave form leaves room for two gather workgroups (2 KB each).
// Prints one line per shape; exit status 0 only if every check holds.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "pgcn_strip_map.h"

using namespace pgcn_strip_map;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (failures < 20) { printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } ++failures; } } while (0)

template <int NW>
static void check() {
    using M = Map<NW>;
    const uint32_t lds0 = 0;
    // ---- 1. pairs --------------------------------------------------------------------------------------------------------------
    const int copy_lanes = NW == 16 ? 32 : 64;
    EXPECT(copy_lanes * 16 == M::kWaveRec, "copy lanes %d", copy_lanes);
    for (int wave = 0; wave < NW; ++wave)
        for (int slot = 0; slot < kRing; ++slot) {
            const uint32_t base = M::ring_slot(lds0, wave, slot);
            EXPECT(base % 16 == 0, "ring slot %u", base);
            EXPECT(M::header(lds0, wave, slot) == base + (uint32_t)M::kWaveRec, "header");
            if (NW == 16) EXPECT(M::header(lds0, wave, slot) == base + 32 * 16, "16 waves: lane 32 of the pair copy brings the header");
            std::vector<int> cover(M::kWaveRec, 0);
            for (int step = 0; step < M::kSteps; ++step)
                for (int gq = 0; gq < 4; ++gq) {
                    const uint32_t a = M::pair_base(lds0, wave, slot, gq) + M::pair_off(step);
                    EXPECT(a % 16 == 0, "pair read %u", a);
                    const int off = (int)(a - base);
                    EXPECT(off >= 0 && off + 16 <= M::kWaveRec, "wave %d step %d gq %d reads offset %d of its slot", wave, step, gq, off);
                    if (off < 0 || off + 16 > M::kWaveRec) continue;
                    for (int b = 0; b < 16; ++b) ++cover[off + b];
                    // the record byte this is (the copy is linear: slot byte o = record byte wave * kWaveRec + o) and the row it belongs to
                    const int rb = wave * M::kWaveRec + off;
                    const int group = rb / kGroupBytes, rowslot = (rb % kGroupBytes) / 16;
                    EXPECT(group == M::row_group(wave, step / kRowSlots, gq), "wave %d step %d gq %d: group %d", wave, step, gq, group);
                    EXPECT(rowslot == step % kRowSlots, "wave %d step %d: row slot %d", wave, step, rowslot);
                    EXPECT(M::local_row(wave, step, gq) == rowslot * kGroups + group, "local row");
                    // the same bytes, groups and steps as the 16-wave kernel's waves 2 W (pass 0) and 2 W + 1 (pass 1)
                    const int w16 = wave * M::kPasses + step / kRowSlots;
                    const int rb16 = w16 * Map<16>::kWaveRec + (int)(Map<16>::pair_base(0, w16, slot, gq) - Map<16>::ring_slot(0, w16, slot)) +
                                     Map<16>::pair_off(step % kRowSlots);
                    EXPECT(rb == rb16 && group == Map<16>::row_group(w16, 0, gq), "wave %d step %d gq %d: record byte %d, 16-wave kernel %d", wave, step, gq, rb, rb16);
                }
            for (int o = 0; o < M::kWaveRec; ++o) EXPECT(cover[o] == 1, "wave %d slot %d: byte %d read %d times", wave, slot, o, cover[o]);
        }
    // every row of the tile is owned once
    {
        std::vector<int> rows(kRows, 0);
        for (int wave = 0; wave < NW; ++wave)
            for (int step = 0; step < M::kSteps; ++step)
                for (int gq = 0; gq < 4; ++gq) ++rows[M::local_row(wave, step, gq)];
        for (int r = 0; r < kRows; ++r) EXPECT(rows[r] == 1, "row %d owned %d times", r, rows[r]);
    }
    // ---- 2. panel copies ---------------------------------------------------------------------------------------------------------
    for (int pb = 0; pb < 2; ++pb) {
        std::vector<int> cover(kPanelBytes, 0);
        for (int q = 0; q < M::kPanelCopies; ++q)
            for (int wave = 0; wave < NW; ++wave)
                for (int lane = 0; lane < 64; ++lane) {
                    const int t = wave * 64 + lane;
                    const int64_t dst = (int64_t)M::panel_dst(lds0, pb, q, wave) + lane * 16 - (int64_t)pb * kPanelBytes;
                    const int row = M::panel_src_row(q) + t / 32, chunk = t % 32;
                    EXPECT(row < kCols, "copy %d thread %d: row %d", q, t, row);
                    EXPECT(dst == (int64_t)row * 512 + chunk * 16, "copy %d thread %d lands at %lld, its row reads expect %d", q, t, (long long)dst, row * 512 + chunk * 16);
                    if (dst < 0 || dst + 16 > kPanelBytes) { EXPECT(false, "copy %d thread %d outside the buffer", q, t); continue; }
                    for (int b = 0; b < 16; ++b) ++cover[dst + b];
                }
        for (int o = 0; o < kCols * 512; ++o) EXPECT(cover[o] == 1, "panel buffer %d: byte %d written %d times", pb, o, cover[o]);
        for (int o = kPadOff; o < kPanelBytes; ++o) EXPECT(cover[o] == 0, "panel buffer %d: the zero row is written at %d", pb, o);
    }
    EXPECT(kPadOff + 512 == kPanelBytes, "the zero row closes a panel buffer");
    // ---- 3. row reads, extents -------------------------------------------------------------------------------------------------------
    for (int pb = 0; pb < 2; ++pb) {
        std::vector<int> cover(512, 0);
        for (int s = 0; s < 16; ++s)
            for (int half = 0; half < 2; ++half) {
                const int64_t o = (int64_t)M::row_base(lds0, pb, s) + half * 256 - (int64_t)pb * kPanelBytes;
                EXPECT(o >= 0 && o + 16 <= 512 && o % 16 == 0, "row read of lane %d at %lld", s, (long long)o);
                if (o >= 0 && o + 16 <= 512) for (int b = 0; b < 16; ++b) ++cover[o + b];
            }
        for (int o = 0; o < 512; ++o) EXPECT(cover[o] == 1, "row byte %d read %d times", o, cover[o]);
    }
    EXPECT(kOffRing == 2 * kPanelBytes && kOffRing % 16 == 0, "rings start behind the two panel buffers");
    uint32_t expect_next = kOffRing;
    for (int wave = 0; wave < NW; ++wave)
        for (int slot = 0; slot < kRing; ++slot) {
            EXPECT(M::ring_slot(lds0, wave, slot) == expect_next, "ring slots are laid end to end");
            expect_next += M::kSlotBytes;
        }
    EXPECT((int)expect_next == M::kSmem, "kSmem %d, the slots end at %u", M::kSmem, expect_next);
    EXPECT(M::kSmem <= kLdsBytes, "%d bytes of LDS", M::kSmem);
    if (NW == 8) EXPECT(kLdsBytes - M::kSmem >= 2 * 2048, "%d bytes left beside an 8-wave workgroup", kLdsBytes - M::kSmem);
    printf("strip map, %2d waves: %d threads, %d steps, %d B of pairs per wave, %d + %d copies, %d B of LDS (%d left)\n", NW, M::kThreads,
           M::kSteps, M::kWaveRec, M::kPanelCopies, M::kPairCopies, M::kSmem, kLdsBytes - M::kSmem);
}

int main() {
    check<16>();
    check<8>();
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
