// pgcn_optim.hip -- one Adam / AdamW step over a flat fp32 parameter arena in ONE launch, for gfx950 (optim.py: FlatAdam).
//
// Per element, in the order of operations of torch.optim.Adam / AdamW (single-tensor path, amsgrad and maximize off), every
// scalar rounded to fp32 where torch's fp32 kernels round theirs:
//
//   gi = g * grad_scale
//   coupled:    gi += weight_decay * p              (only when weight_decay != 0, as torch skips the add)
//   decoupled:  p  *= 1 - lr * weight_decay
//   m += (gi - m) * (1 - beta1)                     (lerp_)
//   v  = beta2 * v + (1 - beta2) * gi * gi          (mul_, addcmul_)
//   denom = sqrt(v) / sqrt(bc2) + eps,  bc1 = 1 - beta1^t,  bc2 = 1 - beta2^t,  t = *step + 1
//   p -= (lr / bc1) * (m / denom)                   (addcdiv_)
//   zero_grad: g = 0 after it was read
//
// The step count is read from device memory (a replayed graph sees the count of ITS replay) and never written here: with
// many blocks that would be a race; the caller adds 1 after the launch.  bc1, bc2, lr / bc1 and sqrt(bc2) are formed in double
// once per thread, before the loop: they are uniform.
//
// Layout: 256 threads, one float4 per lane of each of the four arrays, a grid-stride loop over at most kMaxBlocks blocks --
// one per CU of an MI355X.  The arenas this serves are a model's weights (3 x 128 x 128 floats = 48 blocks): the launch, not
// the sweep, is what such a step costs, so one launch over the padded arena replaces a launch per tensor and per operation;
// a longer arena wraps the loop (four independent 16-byte loads per lane and trip).  The n % 4 last elements take a scalar
// tail; if any base is not 16-byte aligned the scalar loop runs throughout.  Plain vector loads and stores, no LDS, no
// atomics, no allocation, no synchronisation: graph-capturable.
//
// Below it, the step under control (gradient clipping, a learning-rate schedule): pgcn_grad_sumsq_f32 and pgcn_adam_step_ctl_f32,
// the same element function with the learning rate and the gradient factor formed on the device.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "pgcn_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256;

struct AdamArgs {
    double lr, beta1, beta2, eps, weight_decay;
    float grad_scale;
    int32_t decoupled, zero_grad;
};

// the scalars of one step as torch's fp32 kernels see them (Python doubles cast to float at the operation)
struct AdamScalars {
    float gscale, wd, keep, omb1, b2, omb2, sqrt_bc2, eps, step_size;
    bool coupled, decoupled;
};

__device__ __forceinline__ AdamScalars adam_scalars(const AdamArgs &a, const int64_t *__restrict__ step) {
    const double t = (double)(step[0] + 1);
    const double bc1 = 1.0 - pow(a.beta1, t);
    const double bc2 = 1.0 - pow(a.beta2, t);
    AdamScalars s;
    s.gscale = a.grad_scale;
    s.wd = (float)a.weight_decay;
    s.keep = (float)(1.0 - a.lr * a.weight_decay);
    s.omb1 = (float)(1.0 - a.beta1);
    s.b2 = (float)a.beta2;
    s.omb2 = (float)(1.0 - a.beta2);
    s.sqrt_bc2 = (float)sqrt(bc2);
    s.eps = (float)a.eps;
    s.step_size = (float)(a.lr / bc1);
    s.decoupled = a.decoupled != 0;
    s.coupled = !s.decoupled && a.weight_decay != 0.0;
    return s;
}

// One element.  The float4 body and the scalar loop must leave the same bits, so nothing here is left to the compiler's choice of
// contraction (under -ffp-contract=fast the packed body and the scalar loop fused different products): contraction is off, and
// the fused multiply-adds are written out where torch's own kernels have them (add with alpha, lerp_, addcmul_, addcdiv_).
__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, const AdamScalars &s) {
#pragma clang fp contract(off)
    float gi = g * s.gscale;
    if (s.coupled) gi = fmaf(s.wd, p, gi);
    if (s.decoupled) p *= s.keep;
    m = fmaf(gi - m, s.omb1, m);
    v = fmaf(s.omb2 * gi, gi, s.b2 * v);
    const float denom = sqrtf(v) / s.sqrt_bc2 + s.eps;
    p = fmaf(-s.step_size, m / denom, p);
}

// n4: float4 chunks taken by the vector loop (0 when a base is not 16-byte aligned); elements 4 n4 .. n - 1 go one by one
__global__ __launch_bounds__(kThreads) void adam_step_kernel(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m,
                                                             float *__restrict__ v, int64_t n, int64_t n4, AdamArgs a,
                                                             const int64_t *__restrict__ step) {
    const AdamScalars s = adam_scalars(a, step);
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    float4 *p4 = reinterpret_cast<float4 *>(p), *g4 = reinterpret_cast<float4 *>(g);
    float4 *m4 = reinterpret_cast<float4 *>(m), *v4 = reinterpret_cast<float4 *>(v);
    for (int64_t i = tid; i < n4; i += stride) {
        float4 pp = p4[i], mm = m4[i], vv = v4[i];
        const float4 gg = g4[i];
        adam_element(pp.x, gg.x, mm.x, vv.x, s);
        adam_element(pp.y, gg.y, mm.y, vv.y, s);
        adam_element(pp.z, gg.z, mm.z, vv.z, s);
        adam_element(pp.w, gg.w, mm.w, vv.w, s);
        p4[i] = pp;
        m4[i] = mm;
        v4[i] = vv;
        if (a.zero_grad) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int64_t i = 4 * n4 + tid; i < n; i += stride) {
        float pp = p[i], mm = m[i], vv = v[i];
        adam_element(pp, g[i], mm, vv, s);
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
        if (a.zero_grad) g[i] = 0.f;
    }
}

// ---- the step under control: clip coefficient and learning rate formed ON THE DEVICE (optim.py has the definitions) -------------------
//
// pgcn_grad_sumsq_f32: partial[b] = the sum of (double)g * (double)g over the float4 chunks c = b * 256 + lane + trip * parts * 256 of
// g -- chunk c is elements 4 c .. 4 c + 3, the last chunk may be short.  Every product is exact in double (24 x 24 bits), so fused
// or not a sum's bits depend on its order alone: a lane adds its chunks in trip order, x y z w within a chunk, then a fixed LDS tree
// over the 256 lanes.  A chunk is one 16-byte load when the base is 16-byte aligned and it is whole, scalar loads otherwise -- the same
// element reaches the same lane and trip either way, so a misaligned base gives the same bits.  No atomics.
constexpr int64_t kSumsqChunk = 4 * kThreads;          // floats of g per block and trip

__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(const float *__restrict__ g, int64_t n, int64_t n4,
                                                              double *__restrict__ partial) {
    __shared__ double sh[kThreads];
    const int64_t chunks = (n + 3) / 4;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    double acc = 0.0;
    for (int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x; c < chunks; c += stride) {
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        if (c < n4) {
            const float4 q = g4[c];
            e[0] = q.x;
            e[1] = q.y;
            e[2] = q.z;
            e[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * c + j < n) e[j] = g[4 * c + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (double)e[j] * (double)e[j];      // (a missing element adds +0: the sum's bits are unchanged)
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

struct CtlArgs {
    int32_t kind, parts;                                  // 0 constant | 1 cosine | 2 step;  the partial sums (0: no clip)
    double base, warmup, horizon, lr_min, step_every, gamma, max_norm;
};

// lr_at(t, sched) of optim.py in double
__device__ __forceinline__ double lr_at(const CtlArgs &c, double t) {
    double s = c.base;
    if (c.kind == 1) {
        const double u = fmin(fmax((t - c.warmup) / (c.horizon - c.warmup), 0.0), 1.0);
        s = c.lr_min + (c.base - c.lr_min) * 0.5 * (1.0 + cos(M_PI * u));
    } else if (c.kind == 2) {
        s = c.base * pow(c.gamma, floor(fmax(t - c.warmup, 0.0) / c.step_every));
    }
    return t < c.warmup ? s * (t + 1.0) / c.warmup : s;
}

// adam_step_kernel with lr and the gradient factor formed here: every block adds the partial sums in index order (the same bits in
// every block, at most 2 KB), forms coef and lr once per thread, and hands adam_scalars an AdamArgs that holds them.  Block 0
// records {sumsq, norm, coef, lr} in ctl.
__global__ __launch_bounds__(kThreads) void adam_step_ctl_kernel(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m,
                                                                 float *__restrict__ v, int64_t n, int64_t n4, AdamArgs a, CtlArgs c,
                                                                 const double *__restrict__ partial, double *__restrict__ ctl,
                                                                 const int64_t *__restrict__ step) {
    double sumsq = 0.0, norm = 0.0, coef = 1.0;
    if (c.parts > 0) {
        for (int i = 0; i < c.parts; ++i) sumsq += partial[i];
        norm = sqrt(sumsq) * fabs((double)a.grad_scale);
        const double q = c.max_norm / (norm + 1e-6);
        coef = q < 1.0 ? q : (isnan(q) ? q : 1.0);
        a.grad_scale = a.grad_scale * (float)coef;           // one fp32 product; coef == 1: the bits of the unclipped factor
    }
    a.lr = lr_at(c, (double)step[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl[0] = sumsq;
        ctl[1] = norm;
        ctl[2] = coef;
        ctl[3] = a.lr;
    }
    const AdamScalars s = adam_scalars(a, step);
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    float4 *p4 = reinterpret_cast<float4 *>(p), *g4 = reinterpret_cast<float4 *>(g);
    float4 *m4 = reinterpret_cast<float4 *>(m), *v4 = reinterpret_cast<float4 *>(v);
    for (int64_t i = tid; i < n4; i += stride) {
        float4 pp = p4[i], mm = m4[i], vv = v4[i];
        const float4 gg = g4[i];
        adam_element(pp.x, gg.x, mm.x, vv.x, s);
        adam_element(pp.y, gg.y, mm.y, vv.y, s);
        adam_element(pp.z, gg.z, mm.z, vv.z, s);
        adam_element(pp.w, gg.w, mm.w, vv.w, s);
        p4[i] = pp;
        m4[i] = mm;
        v4[i] = vv;
        if (a.zero_grad) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int64_t i = 4 * n4 + tid; i < n; i += stride) {
        float pp = p[i], mm = m[i], vv = v[i];
        adam_element(pp, g[i], mm, vv, s);
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
        if (a.zero_grad) g[i] = 0.f;
    }
}

bool bad_hyper(double x) { return !(x >= 0.0 && x <= DBL_MAX); }      // NaN, negative, infinite

}  // namespace

extern "C" int pgcn_adam_step_f32(float *p, float *g, float *m, float *v, int64_t n, double lr, double beta1, double beta2,
                                  double eps, double weight_decay, int32_t decoupled, float grad_scale, int32_t zero_grad,
                                  const int64_t *step, pgcn_stream_t stream) {
    if (bad_hyper(lr) || bad_hyper(beta1) || bad_hyper(beta2) || bad_hyper(eps) || bad_hyper(weight_decay))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_f32: lr, beta1, beta2, eps and weight_decay must be finite and >= 0");
    if (beta1 >= 1.0 || beta2 >= 1.0) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_f32: beta1 and beta2 must be below 1");
    if (!(fabsf(grad_scale) <= FLT_MAX)) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_f32: grad_scale must be finite");
    if (n < 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_f32: n < 0");
    if (n == 0) return PGCN_OK;
    if (!p || !g || !m || !v || !step) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_f32: null pointer");
    if ((uintptr_t)step % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_f32: step must be 8-byte aligned");
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16) == 0;
    const int64_t n4 = vec ? n / 4 : 0;
    const int64_t work = n4 > 0 ? n4 : n;                   // (the tail of a vector launch is at most 3 elements: one block has them)
    int64_t blocks = (work + kThreads - 1) / kThreads;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    AdamArgs a;
    a.lr = lr;
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.eps = eps;
    a.weight_decay = weight_decay;
    a.grad_scale = grad_scale;
    a.decoupled = decoupled;
    a.zero_grad = zero_grad;
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, p, g, m, v, n, n4, a, step);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int32_t pgcn_grad_sumsq_parts(int64_t n) {
    if (n <= 0) return 0;
    const int64_t parts = (n + kSumsqChunk - 1) / kSumsqChunk;
    return (int32_t)(parts < kMaxBlocks ? parts : kMaxBlocks);
}

extern "C" int pgcn_grad_sumsq_f32(const float *g, int64_t n, double *partial, int32_t parts, pgcn_stream_t stream) {
    if (n < 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_grad_sumsq_f32: n < 0");
    if (parts != pgcn_grad_sumsq_parts(n)) return pgcn_set_error(PGCN_EINVAL, "pgcn_grad_sumsq_f32: parts must be pgcn_grad_sumsq_parts(n)");
    if (n == 0) return PGCN_OK;
    if (!g || !partial) return pgcn_set_error(PGCN_EINVAL, "pgcn_grad_sumsq_f32: null pointer");
    if ((uintptr_t)g % 4 != 0 || (uintptr_t)partial % 8 != 0)
        return pgcn_set_error(PGCN_EINVAL, "pgcn_grad_sumsq_f32: g must be 4-byte and partial 8-byte aligned");
    const int64_t n4 = (uintptr_t)g % 16 == 0 ? n / 4 : 0;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)parts), dim3(kThreads), 0, (hipStream_t)stream, g, n, n4, partial);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}

extern "C" int pgcn_adam_step_ctl_f32(float *p, float *g, float *m, float *v, int64_t n, int32_t kind, double base, double warmup,
                                      double horizon, double lr_min, double step_every, double gamma, double max_norm,
                                      const double *partial, int32_t parts, double *ctl, double beta1, double beta2, double eps,
                                      double weight_decay, int32_t decoupled, float grad_scale, int32_t zero_grad, const int64_t *step,
                                      pgcn_stream_t stream) {
    if (kind < 0 || kind > 2) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: kind takes 0 (constant), 1 (cosine), 2 (step)");
    if (bad_hyper(base) || bad_hyper(warmup) || bad_hyper(horizon) || bad_hyper(lr_min) || bad_hyper(step_every) || bad_hyper(gamma))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: the schedule's values must be finite and >= 0");
    if (kind == 1 && !(horizon > warmup && lr_min <= base))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: cosine needs horizon > warmup and lr_min <= base");
    if (step_every < 1.0) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: step_every < 1");
    if (kind == 2 && !(gamma > 0.0 && gamma <= 1.0)) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: step needs 0 < gamma <= 1");
    if (!(max_norm >= 0.0)) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: max_norm must be >= 0 (0: no clip)");
    if (bad_hyper(beta1) || bad_hyper(beta2) || bad_hyper(eps) || bad_hyper(weight_decay))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: beta1, beta2, eps and weight_decay must be finite and >= 0");
    if (beta1 >= 1.0 || beta2 >= 1.0) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: beta1 and beta2 must be below 1");
    if (!(fabsf(grad_scale) <= FLT_MAX)) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: grad_scale must be finite");
    if (n < 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: n < 0");
    const bool clip = max_norm > 0.0;
    if (!ctl || (uintptr_t)ctl % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: ctl must be a non-null, 8-byte aligned pointer");
    if (!step || (uintptr_t)step % 8 != 0) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: step must be a non-null, 8-byte aligned pointer");
    if (clip && parts != pgcn_grad_sumsq_parts(n))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: parts must be pgcn_grad_sumsq_parts(n) while clipping");
    if (clip && n > 0 && (!partial || (uintptr_t)partial % 8 != 0))
        return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: partial must be a non-null, 8-byte aligned pointer while clipping");
    if (n == 0) return PGCN_OK;
    if (!p || !g || !m || !v) return pgcn_set_error(PGCN_EINVAL, "pgcn_adam_step_ctl_f32: null pointer");
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16) == 0;
    const int64_t n4 = vec ? n / 4 : 0;
    const int64_t work = n4 > 0 ? n4 : n;
    int64_t blocks = (work + kThreads - 1) / kThreads;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    AdamArgs a;
    a.lr = base;                                            // (the kernel puts lr_at(*step) here)
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.eps = eps;
    a.weight_decay = weight_decay;
    a.grad_scale = grad_scale;
    a.decoupled = decoupled;
    a.zero_grad = zero_grad;
    CtlArgs c;
    c.kind = kind;
    c.parts = clip ? parts : 0;
    c.base = base;
    c.warmup = warmup;
    c.horizon = horizon;
    c.lr_min = lr_min;
    c.step_every = step_every;
    c.gamma = gamma;
    c.max_norm = max_norm;
    hipLaunchKernelGGL(adam_step_ctl_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, p, g, m, v, n, n4, a, c,
                       partial, ctl, step);
    PGCN_HIP_CHECK(hipGetLastError());
    return PGCN_OK;
}
