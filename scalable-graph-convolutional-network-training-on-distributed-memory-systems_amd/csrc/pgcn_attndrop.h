// pgcn_attndrop.h -- the keep function of ATTENTION DROPOUT (pgcn_gat_attndrop.hip, include/pgcn_hip.h): whether the normalised
// attention coefficient alpha_ijk of the stored entry (gi attends to gj) and head k survives in training step `step` is a PURE
// FUNCTION of (seed, step, layer, head, the two GLOBAL vertex ids).
//
//   key_l        = dropout_key(seed, step, ATTN_LAYER + layer)      ATTN_LAYER = 1 << 21: reserved, above any layer index (< 2^20)
//                                                                   and above PGCN_EDGE_LAYER (pgcn_dropedge.h)
//   u(gi, gj, k) = dropout_u(dropout_col(key_l, gj), dropout_row(key_l, gi), k + 1)               (gemm/pgcn_dropout.h)
//                = fmix32(fmix32(fmix32(gj ^ lo32(key_l)) ^ gi ^ hi32(key_l)) ^ (k + 1))
//   keep         = u >= thr                                         thr: dropout's threshold of the drop probability
//
// gi: the attending vertex (the row of the softmax), gj: its neighbour, k: the head, 0-based.  NOT symmetric in (gi, gj): alpha_ij
// and alpha_ji are two coefficients.  Self entries are dropped like any other.  dropout_u's third argument is never 0 here, so its
// second round always runs: `attndrop_entry` is what all heads of an entry share, a head costs one fmix32, a compare and a select.
// No dependence on the rank that owns a vertex or on the local numbering: any part vector draws the same mask.
// Ids are below 2^31 (int32 in the structures).
// Plain C++17 without HIP types.  Include gemm/pgcn_dropout.h BEFORE this file (it has no include guard and defines PG_DROPOUT_FN).
// Shared by the kernels, by tests/native/pgcn_attndrop_host.cpp (host build) and restated in integer numpy by dropout.py.
#ifndef PGCN_ATTNDROP_H
#define PGCN_ATTNDROP_H

#define PGCN_ATTN_LAYER (1ull << 21)

PG_DROPOUT_FN uint64_t attndrop_key(uint64_t seed, uint64_t step, uint64_t layer) { return dropout_key(seed, step, PGCN_ATTN_LAYER + layer); }

// the neighbour's share (one value per gj), and what every head of the entry (gi, gj) shares
PG_DROPOUT_FN uint32_t attndrop_col(uint64_t key, uint32_t gj) { return dropout_col(key, gj); }
PG_DROPOUT_FN uint32_t attndrop_entry(uint64_t key, uint32_t a, uint32_t gi) { return dropout_fmix32(a ^ dropout_row(key, (uint64_t)gi)); }
PG_DROPOUT_FN uint32_t attndrop_head(uint32_t b, uint32_t k) { return dropout_fmix32(b ^ (k + 1u)); }

PG_DROPOUT_FN uint32_t attndrop_u(uint64_t key, uint32_t gi, uint32_t gj, uint32_t k) {
    return dropout_u(dropout_col(key, gj), dropout_row(key, (uint64_t)gi), k + 1u);
}

PG_DROPOUT_FN bool attndrop_keep(uint64_t key, uint32_t gi, uint32_t gj, uint32_t k, uint32_t thr) {
    return attndrop_u(key, gi, gj, k) >= thr;
}

#endif
