// pgcn_device.h -- small device helpers shared by the SpMM translation units.
#ifndef PGCN_DEVICE_H
#define PGCN_DEVICE_H
#include <hip/hip_runtime.h>

template <int VEC> struct VecT;
template <> struct VecT<1> { using type = float; };
template <> struct VecT<2> { using type = float2; };
template <> struct VecT<4> { using type = float4; };

template <int VEC>
__device__ __forceinline__ void vload(float (&x)[VEC], const float *p) {
    using V = typename VecT<VEC>::type;
    const V v = *reinterpret_cast<const V *>(p);
    if constexpr (VEC == 1) { x[0] = v; }
    if constexpr (VEC == 2) { x[0] = v.x; x[1] = v.y; }
    if constexpr (VEC == 4) { x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
}

template <int VEC>
__device__ __forceinline__ void vstore(float *p, const float (&x)[VEC]) {
    using V = typename VecT<VEC>::type;
    if constexpr (VEC == 1) { *p = x[0]; }
    if constexpr (VEC == 2) { *reinterpret_cast<V *>(p) = make_float2(x[0], x[1]); }
    if constexpr (VEC == 4) { *reinterpret_cast<V *>(p) = make_float4(x[0], x[1], x[2], x[3]); }
}

// The predicate of the *_if entry points (include/pgcn_hip.h): run_if == NULL -- always run; otherwise one device word that an
// earlier launch on the stream left (pgcn_rows_sync_f32), 0 = the whole launch group is skipped.  The pointer is a kernel argument,
// so the word comes through one wave-uniform scalar load; a kernel calls this before any other memory access and returns on true.
__device__ __forceinline__ bool pgcn_group_off(const int32_t *__restrict__ run_if) {
    return run_if != nullptr && __builtin_amdgcn_readfirstlane(*run_if) == 0;
}
#endif
