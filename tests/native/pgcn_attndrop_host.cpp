// Host build of csrc/pgcn_attndrop.h (the keep function of attention dropout) for tests/test_attndrop.py: the header the kernels
// compile, run entry by entry on the CPU, against the integer-numpy statement in dropout.py (attn_u / attn_keep).
#include <stdint.h>

#define PG_HD static inline
#include "pgcn_dropout.h"
#include "pgcn_attndrop.h"

extern "C" uint64_t pgcn_attndrop_host_key(uint64_t seed, uint64_t step, uint64_t layer) { return attndrop_key(seed, step, layer); }

// u [n x heads] and keep (0 / 1) of n entries (gi[e] attends to gj[e]): once through attndrop_u / attndrop_keep, once through the
// shares the kernels use (attndrop_col, attndrop_entry, attndrop_head); returns the number of words where the two differ
extern "C" int64_t pgcn_attndrop_host_u(uint64_t seed, uint64_t step, uint64_t layer, const int32_t *gi, const int32_t *gj, int64_t n,
                                        int32_t heads, uint32_t thr, uint32_t *u, uint8_t *keep) {
    const uint64_t key = attndrop_key(seed, step, layer);
    int64_t differ = 0;
    for (int64_t e = 0; e < n; ++e) {
        const uint32_t b = attndrop_entry(key, attndrop_col(key, (uint32_t)gj[e]), (uint32_t)gi[e]);
        for (int32_t k = 0; k < heads; ++k) {
            u[e * heads + k] = attndrop_u(key, (uint32_t)gi[e], (uint32_t)gj[e], (uint32_t)k);
            keep[e * heads + k] = attndrop_keep(key, (uint32_t)gi[e], (uint32_t)gj[e], (uint32_t)k, thr) ? 1 : 0;
            differ += attndrop_head(b, (uint32_t)k) != u[e * heads + k];
        }
    }
    return differ;
}
