// pgcn_dropout.h -- the keep function of the fused dropout (gemm/pgcn_dense.hip, include/pgcn_gemm.h): whether element
// (global row, column) of a layer's output survives in training step `step` is a PURE FUNCTION of
// (seed, step, layer, global row id, column).  No generator state, no dependence on which rank owns the row or where it sits in
// that rank's local order: a run on P ranks under any part vector draws the masks of the run on one rank, element for element.
// Plain C++17 without HIP types; PG_HD comes from the including file (device: __device__ __forceinline__, host: static inline).
// Shared by the kernels, by tests/native/pgcn_dropout_host.cpp (host build) and restated in integer numpy by dropout.py.
//
//   mix64(z):  z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
//   key(seed, step, layer) = mix64(mix64(seed) ^ (step * 0x9E3779B97F4A7C15) ^ ((2 layer + 1) * 0xD6E8FEB86659FD93))      (mod 2^64)
//   fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16                                   (mod 2^32)
//   a = fmix32(col ^ lo32(key));  b = fmix32(a ^ lo32(grow) ^ hi32(key));  u = grow < 2^32 ? b : fmix32(b ^ (grow >> 32))
//   keep = u >= thr,  thr = min(floor(p 2^32 + 1/2), 2^32 - 1),  scale = float(1 / (1 - thr / 2^32))  (double division, rounded once)
// The key is pre-mixed so that seeds that differ in one bit do not give column-swapped copies of each other's masks; `a` depends
// on the column only (one value per lane and column block in the kernel), so an element costs one fmix32, a compare and a select.
#ifndef PG_DROPOUT_FN
#define PG_DROPOUT_FN PG_HD          // (the kernel file asks for host AND device copies: the entry points compute the scale)
#endif
PG_DROPOUT_FN uint64_t dropout_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
PG_DROPOUT_FN uint64_t dropout_key(uint64_t seed, uint64_t step, uint64_t layer) {
    return dropout_mix64(dropout_mix64(seed) ^ (step * 0x9E3779B97F4A7C15ull) ^ ((2 * layer + 1) * 0xD6E8FEB86659FD93ull));
}
PG_DROPOUT_FN uint32_t dropout_fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}
// the column's share of the hash
PG_DROPOUT_FN uint32_t dropout_col(uint64_t key, uint32_t col) { return dropout_fmix32(col ^ (uint32_t)key); }
// the row's share, folded with the key's high half: what is XOR-ed into `a` (one value per row, the same for every column)
PG_DROPOUT_FN uint32_t dropout_row(uint64_t key, uint64_t grow) { return (uint32_t)grow ^ (uint32_t)(key >> 32); }
// u of an element from the two shares; row_hi = grow >> 32 (0 for ids below 2^32: no second round)
PG_DROPOUT_FN uint32_t dropout_u(uint32_t a, uint32_t row_term, uint32_t row_hi) {
    const uint32_t b = dropout_fmix32(a ^ row_term);
    return row_hi ? dropout_fmix32(b ^ row_hi) : b;
}
PG_DROPOUT_FN bool dropout_keep(uint64_t key, uint64_t grow, uint32_t col, uint32_t thr) {
    return dropout_u(dropout_col(key, col), dropout_row(key, grow), (uint32_t)(grow >> 32)) >= thr;
}
// 1 / (1 - thr / 2^32) as the float every implementation multiplies by
PG_DROPOUT_FN float dropout_scale(uint32_t thr) { return (float)(1.0 / (1.0 - (double)thr / 4294967296.0)); }
