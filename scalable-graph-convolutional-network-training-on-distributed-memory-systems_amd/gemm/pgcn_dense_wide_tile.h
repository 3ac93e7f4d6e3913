// pgcn_dense_wide_tile.h -- the index arithmetic of gemm/pgcn_dense_wide.hip beside pgcn_dense_tile.h (which it builds on: slots,
// windows, pieces, accumulator rows and the sign-mask words are the narrow kernel's): the CHUNKED image of B operands in the
// caller's work-space, the split of a row panel and of the weight gradient's rows, the argument checks.
// Included INSIDE namespace pgcn_dense_wide AFTER pgcn_dense_tile.h; PG_HD comes from the including file.
//
// Image.  Bm (K x N; W^T for the forward, W for the input gradient) is cut into CHUNKS of 64 x 128 = 4 k steps x 4 column blocks.
// A chunk is the narrow image restricted to those steps and blocks, contiguous:
//     chunk[plane p][k step ks][column block nb][lane] x 16 B  = 3 x 16 KB = 48 KB,
// the eight bf16 of a slot being Bm[64 kc + 16 ks + 8 (lane >> 5) + j][128 np + 32 nb + (lane & 31)], zero outside K x N.  The chunks
// of one column panel np follow each other in k: chunk (np, kc) sits at (np * nkc + kc) * 48 KB, which is the order the kernel
// consumes them in.
constexpr int kWideMinF = 4;
constexpr int kWideMaxF = 1024;
constexpr int kPanelRows = kRows * kWaves;                  // 256 rows of a workgroup
constexpr int kChunkK = 64, kChunkN = 128;                  // 4 k steps x 4 column blocks
constexpr int kChunkSlots = 4 * 4 * 64;                     // (k step, column block, lane) per plane
constexpr int kChunkPlaneBytes = kChunkSlots * 16;          // 16 KB
constexpr int kChunkBytes = 3 * kChunkPlaneBytes;           // 48 KB
constexpr int kRingBytes = 2 * kChunkBytes;                 // the two-slot LDS ring: 96 KB
constexpr int kWaveShare = kChunkBytes / kWaves;            // bytes of a chunk that one wave copies: 6 KB = 6 x (64 lanes x 16 B)

constexpr int chunks_k(int K) { return (K + kChunkK - 1) / kChunkK; }
constexpr int panels_n(int N) { return (N + kChunkN - 1) / kChunkN; }
constexpr int64_t chunk_base(int np, int kc, int nkc) { return ((int64_t)np * nkc + kc) * kChunkBytes; }
// byte offset of a lane's B operand inside a chunk (the order of image_offset: plane, k step, column block, lane)
constexpr int chunk_offset(int plane, int ks, int nb, int lane) { return plane * kChunkPlaneBytes + ((ks * 4 + nb) * 64 + lane) * 16; }
inline int64_t image_bytes(int K, int N) { return (int64_t)chunks_k(K) * panels_n(N) * kChunkBytes; }

// ---- the weight gradient's work items -----------------------------------------------------------------------------------------------
// dW (fout x fin) is cut into TO x TK tiles of 64 x 64 (at most 16 x 16), the n rows into 16-row steps and those into `ranges`
// contiguous row ranges; a wave owns one (range, tile).  The number of ranges is a function of the SHAPE alone (the work-space size
// must be known without a device, and the order of the sums must not depend on one):
//     ranges = clamp(kWgradWaves / tiles, 1, max(1, steps / kWgradMinSteps))
// kWgradWaves = 2048 work items fill a chip of 256 CUs with one 8-wave workgroup each; a range keeps at least four steps; the
// work-space, ranges x (64 TO) x (64 TK) floats, stays at or below 2048 x 4096 floats = 32 MB whatever the widths.
constexpr int kWgradWaves = 2048;
constexpr int kWgradMinSteps = 4;
constexpr int kStepRows = 16;
inline int wgrad_tiles(int f) { return (f + 63) / 64; }
inline int wgrad_ranges(int64_t n, int fout, int fin) {
    const int64_t steps = (n + kStepRows - 1) / kStepRows;
    int64_t r = kWgradWaves / (wgrad_tiles(fout) * wgrad_tiles(fin));
    const int64_t most = steps / kWgradMinSteps;
    if (r > most) r = most;
    return (int)(r < 1 ? 1 : r);
}

// ---- argument checks: every shape has one owner -------------------------------------------------------------------------------------
inline int check_widths(int fin, int fout) {
    if (fin <= 0 || fout <= 0) return fail(-1, "pgcn_dense_wide: bad argument");
    if (fin % 4 || fout % 4 || fin < kWideMinF || fout < kWideMinF || fin > kWideMaxF || fout > kWideMaxF)
        return fail(-2, "pgcn_dense_wide: widths must be multiples of 4 in 4 .. 1024");
    if (fin <= kMaxF && fout <= kMaxF) return fail(-2, "pgcn_dense_wide: widths up to 128 belong to the narrow kernels");
    return 0;
}
// a streamed operand or result: 16-byte pieces, a leading dimension that a tile's 32-bit lane offsets can hold
inline int check_streamed(const void *M, int64_t ld, int width) {
    if (ld < width) return fail(-1, "pgcn_dense_wide: leading dimension below the width");
    if (ld % 4 || (uintptr_t)M % 16) return fail(-2, "pgcn_dense_wide: rows of a streamed operand must be 16-byte pieces");
    return check_ld(ld);
}
