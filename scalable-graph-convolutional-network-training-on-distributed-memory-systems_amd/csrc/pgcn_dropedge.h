// pgcn_dropedge.h -- the keep function of DropEdge (pgcn_dropedge.hip, include/pgcn_hip.h): whether the stored entry (gi, gj) of
// the adjacency pattern survives in training step `step` is a PURE FUNCTION of (seed, step, the two GLOBAL vertex ids).
//
//   key_E        = dropout_key(seed, step, EDGE_LAYER)          EDGE_LAYER = 1 << 20: reserved, above any layer index
//   u(gi, gj)    = dropout_u of (key_E, grow = min(gi, gj), col = max(gi, gj))      (gemm/pgcn_dropout.h: the hash of feature dropout)
//   keep(gi, gj) = gi == gj  ||  u(gi, gj) >= thr               thr: dropout's threshold of the drop probability
//
// Symmetric in (gi, gj): an undirected edge goes or stays in both directions, and the transposed structure sees the mask of the
// forward one.  Self loops always stay, so every vertex of A + I keeps a degree of at least 1.  One mask serves all layers of a
// step.  No dependence on the rank that owns a vertex or on the local numbering: any part vector draws the same mask.
// Ids are below 2^31 (int32 in the structures), so the hash never takes its second round.
// Plain C++17 without HIP types.  Include gemm/pgcn_dropout.h BEFORE this file (it has no include guard and defines PG_DROPOUT_FN).
// Shared by the kernels, by tests/native/pgcn_dropedge_host.cpp (host build) and restated in integer numpy by dropout.py.
#ifndef PGCN_DROPEDGE_H
#define PGCN_DROPEDGE_H

#define PGCN_EDGE_LAYER (1ull << 20)

PG_DROPOUT_FN uint64_t dropedge_key(uint64_t seed, uint64_t step) { return dropout_key(seed, step, PGCN_EDGE_LAYER); }

PG_DROPOUT_FN uint32_t dropedge_u(uint64_t key, uint32_t gi, uint32_t gj) {
    const uint32_t lo = gi < gj ? gi : gj, hi = gi < gj ? gj : gi;
    return dropout_u(dropout_col(key, hi), dropout_row(key, (uint64_t)lo), 0u);
}

PG_DROPOUT_FN bool dropedge_keep(uint64_t key, uint32_t gi, uint32_t gj, uint32_t thr) {
    return gi == gj || dropedge_u(key, gi, gj) >= thr;
}

#endif
