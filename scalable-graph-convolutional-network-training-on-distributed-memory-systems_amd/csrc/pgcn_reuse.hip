// pgcn_reuse.hip -- has an operand changed since its aggregation was kept?  Decided on the device, from the operand's bits, for gfx950
// (engine.py: AggregationEngine.forward_reusing; include/pgcn_hip.h has the contract).
//
//   pgcn_rows_sync_f32   one pass over H and a kept copy `ref`: the elements are compared as 32-bit patterns (-0 differs from +0, a NaN
//                        equals itself only with the same payload); where they differ -- everywhere if force != 0 -- ref = H.
//                        changed[0] = 1 if anything differed or force was set, else 0.
//
// The word is what the *_if entry points of the sum path's launch group take as run_if: 0 = the kept aggregation of `ref` is still the
// aggregation of H, and every workgroup of the group returns at once.  Two launches: a one-thread kernel that sets the word (so it is
// cleared by this call itself, in stream order, not by a memset), then the compare, whose workgroups store a 1 where they saw a
// difference -- every writer of the word after the first kernel stores the same value.  Raw pointers + a stream, no allocation, no
// synchronisation, plain vector stores: graph-capturable.  Cost: 2 * nrows * f * 4 bytes read (238.6 MB at 232 965 x 128), and
// nothing written while the operand stays the same.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgcn_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kInFlight = 4;          // units of H and of ref a thread has in flight: 8 loads issued back to back
constexpr int64_t kMaxBlocks = 2048;  // 8 workgroups of 256 threads per CU on 256 CUs; the loop strides over the rest

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

__global__ void sync_flag_kernel(int32_t *__restrict__ changed, int32_t value) { changed[0] = value; }

template <int VEC> struct Unit;
template <> struct Unit<4> { using type = u32x4; };
template <> struct Unit<1> { using type = uint32_t; };

__device__ __forceinline__ bool differs(u32x4 a, u32x4 b) { return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) != 0; }
__device__ __forceinline__ bool differs(uint32_t a, uint32_t b) { return a != b; }

// A matrix of nrows x (upr units of VEC words), leading dimensions in words.  FLAT: one run of `total` units (contiguous operands),
// no row arithmetic.  Unit u of the matrix is row u / upr, columns VEC (u % upr) ..; every offset is 64-bit.
template <int VEC, bool FLAT>
__global__ __launch_bounds__(kThreads) void rows_sync_kernel(const uint32_t *__restrict__ H, int64_t ldh, uint32_t *__restrict__ ref,
                                                             int64_t ldr, int64_t total, int64_t upr, int force,
                                                             int32_t *__restrict__ changed) {
    using U = typename Unit<VEC>::type;
    const int64_t nthreads = (int64_t)gridDim.x * kThreads;
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    bool any = false;
    for (int64_t u0 = tid; u0 < total; u0 += kInFlight * nthreads) {
        U h[kInFlight], r[kInFlight];
        int64_t oh[kInFlight], orf[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const int64_t u = u0 + k * nthreads;
            if (FLAT) {
                oh[k] = orf[k] = u * VEC;
            } else {
                const int64_t row = u / upr, c = (u - row * upr) * VEC;
                oh[k] = row * ldh + c;
                orf[k] = row * ldr + c;
            }
        }
#pragma unroll
        for (int k = 0; k < kInFlight; ++k)
            if (u0 + k * nthreads < total) h[k] = *reinterpret_cast<const U *>(H + oh[k]);
#pragma unroll
        for (int k = 0; k < kInFlight; ++k)
            if (u0 + k * nthreads < total) r[k] = *reinterpret_cast<const U *>(ref + orf[k]);
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            if (u0 + k * nthreads >= total) break;
            const bool d = differs(h[k], r[k]);
            any = any || d;
            if (d || force) *reinterpret_cast<U *>(ref + orf[k]) = h[k];
        }
    }
    if (__syncthreads_or(any) && threadIdx.x == 0) changed[0] = 1;
}

template <int VEC, bool FLAT>
void launch_sync(const uint32_t *H, int64_t ldh, uint32_t *ref, int64_t ldr, int64_t total, int64_t upr, int force, int32_t *changed,
                 hipStream_t s) {
    const int64_t per_block = (int64_t)kThreads * kInFlight;
    int64_t blocks = (total + per_block - 1) / per_block;
    blocks = blocks < kMaxBlocks ? blocks : kMaxBlocks;
    hipLaunchKernelGGL((rows_sync_kernel<VEC, FLAT>), dim3((unsigned)blocks), dim3(kThreads), 0, s, H, ldh, ref, ldr, total, upr, force,
                       changed);
}

bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" int pgcn_rows_sync_f32(const float *H, int64_t ldh, float *ref, int64_t ldr, int64_t nrows, int32_t f, int32_t force,
                                  int32_t *changed, pgcn_stream_t stream) {
    if (nrows < 0 || f < 1) return pgcn_set_error(PGCN_EINVAL, "pgcn_rows_sync_f32: nrows < 0 or f < 1");
    if (!changed) return pgcn_set_error(PGCN_EINVAL, "pgcn_rows_sync_f32: changed is NULL");
    if (nrows > 0 && (!H || !ref)) return pgcn_set_error(PGCN_EINVAL, "pgcn_rows_sync_f32: null pointer");
    if (ldh < f || ldr < f) return pgcn_set_error(PGCN_EINVAL, "pgcn_rows_sync_f32: a leading dimension is below f");
    if (nrows > 0 && (const float *)ref == H) return pgcn_set_error(PGCN_EINVAL, "pgcn_rows_sync_f32: ref is H itself");
    hipStream_t s = (hipStream_t)stream;
    const int fc = force != 0;
    hipLaunchKernelGGL(sync_flag_kernel, dim3(1), dim3(1), 0, s, changed, (int32_t)fc);
    PGCN_HIP_CHECK(hipGetLastError());
    if (nrows == 0) return PGCN_OK;
    const uint32_t *h = reinterpret_cast<const uint32_t *>(H);
    uint32_t *r = reinterpret_cast<uint32_t *>(ref);
    const bool al = aligned16(H) && aligned16(ref);
    if (ldh == f && ldr == f) {            // contiguous: one run of nrows * f words, 16-byte units and a scalar tail of < 4 words
        const int64_t total = nrows * (int64_t)f;
        const int64_t quads = al ? total / 4 : 0, done = quads * 4;
        if (quads > 0) launch_sync<4, true>(h, 0, r, 0, quads, 0, fc, changed, s);
        if (total > done) launch_sync<1, true>(h + done, 0, r + done, 0, total - done, 0, fc, changed, s);
    } else if (al && f % 4 == 0 && ldh % 4 == 0 && ldr % 4 == 0) {
        launch_sync<4, false>(h, ldh, r, ldr, nrows * (int64_t)(f / 4), f / 4, fc, changed, s);
    } else {
        launch_sync<1, false>(h, ldh, r, ldr, nrows * (int64_t)f, f, fc, changed, s);
    }
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}
