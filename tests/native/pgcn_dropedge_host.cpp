// Host build of csrc/pgcn_dropedge.h (the keep function of DropEdge) for tests/test_dropedge.py: the header the kernels compile, run
// entry by entry on the CPU, against the integer-numpy statement in dropout.py (edge_u / edge_keep).
#include <stdint.h>

#define PG_HD static inline
#include "pgcn_dropout.h"
#include "pgcn_dropedge.h"

extern "C" uint64_t pgcn_dropedge_host_key(uint64_t seed, uint64_t step) { return dropedge_key(seed, step); }

// u and keep (0 / 1) of n entries (gi[k], gj[k])
extern "C" void pgcn_dropedge_host_u(uint64_t seed, uint64_t step, const int32_t *gi, const int32_t *gj, int64_t n, uint32_t thr,
                                     uint32_t *u, uint8_t *keep) {
    const uint64_t key = dropedge_key(seed, step);
    for (int64_t k = 0; k < n; ++k) {
        u[k] = dropedge_u(key, (uint32_t)gi[k], (uint32_t)gj[k]);
        keep[k] = dropedge_keep(key, (uint32_t)gi[k], (uint32_t)gj[k], thr) ? 1 : 0;
    }
}
