// Host build of gemm/pgcn_dropout.h (the keep function of the fused dropout) for tests/test_dropout.py: the header the kernels
// compile, run element by element on the CPU, against the integer-numpy statement in dropout.py.
#include <stdint.h>

#define PG_HD static inline
#include "pgcn_dropout.h"

extern "C" uint64_t pgcn_dropout_host_key(uint64_t seed, uint64_t step, uint64_t layer) { return dropout_key(seed, step, layer); }

extern "C" float pgcn_dropout_host_scale(uint32_t thr) { return dropout_scale(thr); }

// keep (n x width bytes, 0 / 1) of rows `row_ids` (NULL: the row index)
extern "C" void pgcn_dropout_host_keep(uint64_t seed, uint64_t step, uint64_t layer, const int64_t *row_ids, int64_t n, int32_t width,
                                       uint32_t thr, uint8_t *keep) {
    const uint64_t key = dropout_key(seed, step, layer);
    for (int64_t i = 0; i < n; ++i)
        for (int32_t c = 0; c < width; ++c)
            keep[i * width + c] = dropout_keep(key, row_ids ? (uint64_t)row_ids[i] : (uint64_t)i, (uint32_t)c, thr) ? 1 : 0;
}
