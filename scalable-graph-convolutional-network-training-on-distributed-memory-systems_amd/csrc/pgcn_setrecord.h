// pgcn_setrecord.h -- the per-set record of the masked losses (pgcn_loss.hip, pgcn_loss_multilabel.hip): what a lane gathers over
// the rows it leads, the block's partial record, the kernel that adds the partial records, and the host-side checks around
// them.  Header-only, everything in an anonymous namespace: each translation unit keeps its own copy under its own compile flags.
//
// One layout with P count planes, every field indexed by the split code (slot 0 = rows in no set: counted in `rows`, zero
// elsewhere):   double loss_sum[4];  int64 plane[P][4];  int64 rows[4]         = 4 (2 + P) 8-byte words
//   P = 1  pgcn_masked_nll_stats  (correct)            P = 3  pgcn_masked_bce_stats  (tp, fp, fn)
//
// A block owns kSetRows = 64 consecutive rows and writes ONE partial record to the work-space; a second, one-block launch adds
// the records.  Every double sum has a fixed order -- per lane over its rows; butterfly 32 .. 1 over the wave; waves 0 .. 3; in
// the second launch thread t takes records t, t + 256, ..., then the same butterfly and wave order -- no floating-point atomics,
// two calls give the same bits.  (The counts are integers: exact in any order.)  Every barrier is reached by the whole block.
#ifndef PGCN_SETRECORD_H
#define PGCN_SETRECORD_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgcn_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSetRows = 64;             // rows per block of a masked forward: one partial record per 64 rows

// what one lane has seen of the rows it leads
template <int P>
struct SetRecord {
    static constexpr int kWords = 4 * (2 + P);
    static constexpr int kCounts = 3 * P + 4;            // plane[p][1..3] at 3 p, rows[0..3] at 3 P
    double loss[3];
    int cnt[P][3];
    int rows[4];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            loss[s] = 0.0;
#pragma unroll
            for (int p = 0; p < P; ++p) cnt[p][s] = 0;
        }
        rows[0] = rows[1] = rows[2] = rows[3] = 0;
    }
    // selects, not products: a NaN row loss reaches its own set only
    __device__ __forceinline__ void add(int k, float row_loss, const int (&c)[P]) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const bool mine = k == s + 1;
            loss[s] += mine ? (double)row_loss : 0.0;
#pragma unroll
            for (int p = 0; p < P; ++p) cnt[p][s] += mine ? c[p] : 0;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) rows[s] += (k == s) ? 1 : 0;
    }
    // butterfly over the wave, then the block's four waves in order: one record per block, fixed order
    __device__ __forceinline__ void block_store(unsigned long long *__restrict__ part) {
        __shared__ double s_loss[kThreads / 64][3];
        __shared__ int s_cnt[kThreads / 64][kCounts];
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                loss[s] += __shfl_xor(loss[s], o, 64);
#pragma unroll
                for (int p = 0; p < P; ++p) cnt[p][s] += __shfl_xor(cnt[p][s], o, 64);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) rows[s] += __shfl_xor(rows[s], o, 64);
        }
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                s_loss[w][s] = loss[s];
#pragma unroll
                for (int p = 0; p < P; ++p) s_cnt[w][3 * p + s] = cnt[p][s];
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) s_cnt[w][3 * P + s] = rows[s];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double *pl = reinterpret_cast<double *>(part + (size_t)blockIdx.x * kWords);
            long long *pc = reinterpret_cast<long long *>(part + (size_t)blockIdx.x * kWords) + 4;
            pl[0] = 0.0;
            for (int s = 0; s < 3; ++s) {
                double a = s_loss[0][s];
                for (int v = 1; v < kThreads / 64; ++v) a += s_loss[v][s];
                pl[1 + s] = a;
            }
            for (int p = 0; p < P; ++p) {                     // the count planes: slot 0 is zero
                pc[4 * p] = 0;
                for (int s = 0; s < 3; ++s) {
                    long long c = s_cnt[0][3 * p + s];
                    for (int v = 1; v < kThreads / 64; ++v) c += s_cnt[v][3 * p + s];
                    pc[4 * p + 1 + s] = c;
                }
            }
            for (int s = 0; s < 4; ++s) {
                long long c = s_cnt[0][3 * P + s];
                for (int v = 1; v < kThreads / 64; ++v) c += s_cnt[v][3 * P + s];
                pc[4 * P + s] = c;
            }
        }
    }
};

__device__ __forceinline__ int split_code(const uint8_t *__restrict__ split, int64_t i) {
    const int s = split[i];
    return s <= 3 ? s : 0;
}

// one block: thread t adds records t, t + 256, ... in that order, then the same butterfly / wave order as above
template <int P>
__global__ __launch_bounds__(kThreads) void set_finalize_kernel(const unsigned long long *__restrict__ part, int64_t nblocks,
                                                                unsigned long long *__restrict__ stats) {
    constexpr int kWords = SetRecord<P>::kWords, kCounts = SetRecord<P>::kCounts;
    __shared__ double s_loss[kThreads / 64][3];
    __shared__ long long s_cnt[kThreads / 64][kCounts];
    double loss[3] = {0.0, 0.0, 0.0};
    long long cnt[kCounts];
#pragma unroll
    for (int s = 0; s < kCounts; ++s) cnt[s] = 0;
    for (int64_t b = threadIdx.x; b < nblocks; b += kThreads) {
        const double *pl = reinterpret_cast<const double *>(part + b * kWords);
        const long long *pc = reinterpret_cast<const long long *>(part + b * kWords) + 4;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            loss[s] += pl[1 + s];
#pragma unroll
            for (int p = 0; p < P; ++p) cnt[3 * p + s] += pc[4 * p + 1 + s];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) cnt[3 * P + s] += pc[4 * P + s];
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int s = 0; s < 3; ++s) loss[s] += __shfl_xor(loss[s], o, 64);
#pragma unroll
        for (int s = 0; s < kCounts; ++s) cnt[s] += __shfl_xor(cnt[s], o, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int s = 0; s < 3; ++s) s_loss[w][s] = loss[s];
#pragma unroll
        for (int s = 0; s < kCounts; ++s) s_cnt[w][s] = cnt[s];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *ol = reinterpret_cast<double *>(stats);
        long long *oc = reinterpret_cast<long long *>(stats) + 4;
        ol[0] = 0.0;
        for (int s = 0; s < 3; ++s) {
            double a = s_loss[0][s];
            for (int v = 1; v < kThreads / 64; ++v) a += s_loss[v][s];
            ol[1 + s] = a;
        }
        for (int p = 0; p < P; ++p) {
            oc[4 * p] = 0;
            for (int s = 0; s < 3; ++s) {
                long long c = s_cnt[0][3 * p + s];
                for (int v = 1; v < kThreads / 64; ++v) c += s_cnt[v][3 * p + s];
                oc[4 * p + 1 + s] = c;
            }
        }
        for (int s = 0; s < 4; ++s) {
            long long c = s_cnt[0][3 * P + s];
            for (int v = 1; v < kThreads / 64; ++v) c += s_cnt[v][3 * P + s];
            oc[4 * P + s] = c;
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
template <int P>
int64_t set_ws_bytes(int64_t nrows) {
    const int64_t blocks = nrows > 0 ? (nrows + kSetRows - 1) / kSetRows : 1;
    return blocks * SetRecord<P>::kWords * (int64_t)sizeof(unsigned long long);
}

// the record's own checks, in the entry point `name`; leaves the number of partial records in *blocks
inline int set_check_record(const char *name, const void *stats, int64_t nrows, int64_t *blocks) {
    if (!stats || (uintptr_t)stats % 8 != 0) return pgcn_set_error2(PGCN_EINVAL, name, "stats must be 8-byte aligned");
    *blocks = (nrows + kSetRows - 1) / kSetRows;
    if (*blocks > 0x7fffffffLL) return pgcn_set_error2(PGCN_EINVAL, name, "too many rows");
    return PGCN_OK;
}

template <int P>
int set_check_ws(const char *name, const void *ws, int64_t ws_bytes, int64_t nrows) {
    if (!ws || (uintptr_t)ws % 8 != 0 || ws_bytes < set_ws_bytes<P>(nrows))
        return pgcn_set_error2(PGCN_EINVAL, name, "work-space too small or not 8-byte aligned");
    return PGCN_OK;
}

// adds the `blocks` partial records of `ws` into *stats (no rows: the record is still written -- all zeros)
template <int P>
int set_finalize(const void *ws, int64_t blocks, void *stats, pgcn_stream_t stream) {
    hipLaunchKernelGGL(set_finalize_kernel<P>, dim3(1), dim3(kThreads), 0, (hipStream_t)stream,
                       static_cast<const unsigned long long *>(ws), blocks, static_cast<unsigned long long *>(stats));
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

}  // namespace

#endif
