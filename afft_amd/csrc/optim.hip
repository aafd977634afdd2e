// Adam / AdamW over the flat parameter buffers (include/afft_hip.h: afft_adam, afft_adam_runs).  HBM-bound: 30 B per parameter
// with a bf16 image (p, m, v read and written, fp32 gradient read, bf16 image written), 33 B with the fp16 and e4m3 images too.
// Behind them the weight average over the same buffers (afft_ema: 12 B per parameter) and the exact exchange that puts the average
// in the parameters' place for an evaluation (afft_swap_f32: 16 B per element).
#include <climits>
#include <cmath>
#include <cstdlib>

#include "common.h"

namespace {

// per-launch constants of the update: the bias corrections are computed once per thread, in double precision, from the step
// counter the host advances (afft_adam: the kernels never write it, so a skipped step does not advance them)
struct AdamCoef {
  float b1, b2, omb1, omb2, eps, wd, decay, step_size, bc2_sqrt, gscale;
  int decoupled;
};

__device__ __forceinline__ AdamCoef adam_coef(float lr, float b1, float b2, float eps, float wd, float gscale,
                                              const float* __restrict__ step_dev, int flags) {
  const double t = (double)*step_dev + 1.0;
  AdamCoef c;
  c.b1 = b1;
  c.b2 = b2;
  c.omb1 = 1.0f - b1;
  c.omb2 = 1.0f - b2;
  c.eps = eps;
  c.wd = wd;
  c.decay = (float)(1.0 - (double)lr * (double)wd);
  c.step_size = (float)((double)lr / (1.0 - pow((double)b1, t)));
  c.bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, t));
  c.gscale = gscale;
  c.decoupled = flags & AFFT_ADAM_DECOUPLED;
  return c;
}

// one element, shared by both kernels: every rounding is pinned (explicit fma / mul / div / sqrt), so the flat and the runs
// kernel -- and the 4-wide and scalar paths of the flat one -- give bit-identical parameters, moments and images
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, const AdamCoef& c) {
  g = __fmul_rn(g, c.gscale);
  if (c.decoupled) p = __fmul_rn(p, c.decay);
  else g = __fmaf_rn(c.wd, p, g);
  m = __fmaf_rn(c.b1, m, __fmul_rn(c.omb1, g));
  v = __fmaf_rn(c.b2, v, __fmul_rn(__fmul_rn(c.omb2, g), g));
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), c.bc2_sqrt), c.eps);
  p = __fmaf_rn(-c.step_size, __fdiv_rn(m, denom), p);
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const void* __restrict__ g_, int g_dtype,
                                                   float* __restrict__ m, float* __restrict__ v, bf16_t* __restrict__ p16,
                                                   bf16_t* __restrict__ p16h, unsigned char* __restrict__ p8, int64_t n, float lr,
                                                   float b1, float b2, float eps, float wd, float gscale,
                                                   const float* __restrict__ gscale_dev, const float* __restrict__ step_dev,
                                                   int flags, const float* __restrict__ ok) {
  if (ok && *ok == 0.f) return;            // non-finite loss: the step is a no-op (afft_sgd_fused_t.ok)
  if (gscale_dev) gscale *= *gscale_dev;   // clip coefficient computed on the device (afft_clip_coef)
  const AdamCoef c = adam_coef(lr, b1, b2, eps, wd, gscale, step_dev, flags);
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * 1024) {
    if (i + 3 < n) {
      const float4 pv = *(const float4*)(p + i);
      const float4 mv = *(const float4*)(m + i);
      const float4 vv = *(const float4*)(v + i);
      float gg[4];
      load4(g_, i, g_dtype, gg);
      float pp[4] = {pv.x, pv.y, pv.z, pv.w};
      float mm[4] = {mv.x, mv.y, mv.z, mv.w};
      float qq[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) adam_update(pp[r], mm[r], qq[r], gg[r], c);
      *(float4*)(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
      *(float4*)(v + i) = make_float4(qq[0], qq[1], qq[2], qq[3]);
      *(float4*)(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
      if (p16) store4(p16, i, AFFT_BF16, pp);
      if (p16h) store4(p16h, i, AFFT_F16, pp);
      if (p8) store_e4m3<4>(p8, i, pp, 256.0f);
    } else {
      for (int64_t j = i; j < n; ++j) {
        float pj = p[j], mj = m[j], vj = v[j];
        adam_update(pj, mj, vj, ld_any(g_, j, g_dtype), c);
        m[j] = mj;
        v[j] = vj;
        p[j] = pj;
        if (p16) p16[j] = f2bf(pj);
        if (p16h) p16h[j] = f2h(pj);
        if (p8) p8[j] = f2e4m3(pj * 256.0f);
      }
    }
  }
}

// the same update over a table of runs {start, length}: block b owns run b (runs are <= 16 Ki elements: parallel.FusedAdam)
__global__ __launch_bounds__(256) void adam_runs_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, bf16_t* __restrict__ p16, bf16_t* __restrict__ p16h,
                                                        unsigned char* __restrict__ p8, const int64_t* __restrict__ runs, float lr,
                                                        float b1, float b2, float eps, float wd, float gscale,
                                                        const float* __restrict__ step_dev, int flags, const float* __restrict__ ok) {
  if (ok && *ok == 0.f) return;
  const AdamCoef c = adam_coef(lr, b1, b2, eps, wd, gscale, step_dev, flags);
  const int64_t s0 = runs[2 * blockIdx.x], len = runs[2 * blockIdx.x + 1];
  for (int64_t j = s0 + threadIdx.x; j < s0 + len; j += 256) {
    float pj = p[j], mj = m[j], vj = v[j];
    adam_update(pj, mj, vj, g[j], c);
    m[j] = mj;
    v[j] = vj;
    p[j] = pj;
    if (p16) p16[j] = f2bf(pj);
    if (p16h) p16h[j] = f2h(pj);
    if (p8) p8[j] = f2e4m3(pj * 256.0f);
  }
}

// ---- weight averaging (include/afft_hip.h: afft_ema, afft_swap_f32).  Two streams in, one or two out, nothing to compute: what
//      decides the rate is the bytes in flight.  The grid is adam_kernel's (one 256-thread block per CU under the same cap), so every
//      thread keeps kStreamUnroll 16-byte loads per stream in flight -- a block stride apart, so that a wave's access stays one
//      contiguous KiB -- where adam_kernel's four streams make do with one each.
constexpr int kStreamUnroll = 4;

// one element: every rounding is pinned (one subtraction, one fma), so the 16-byte and the element paths give the same bits.
// d == 0 keeps e itself: fma(w, +0, -0) would turn a negative zero into a positive one.
__device__ __forceinline__ float ema_update(float e, float p, float w) {
  const float d = __fsub_rn(p, e);
  const float r = __fmaf_rn(w, d, e);
  return d == 0.f ? e : r;
}
// (f32x4, the compiler's own vector type: through HIP's float4 struct the accesses came out as 8-byte halves)
__device__ __forceinline__ f32x4 ema_update4(const f32x4 e, const f32x4 p, float w) {
  f32x4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = ema_update(e[k], p[k], w);
  return r;
}

// both bases 16-byte aligned: whole 16-byte groups in the body, the n % 4 elements behind them one lane each
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n, float w,
                                                  const float* __restrict__ ok) {
  if (ok && *ok == 0.f) return;            // the optimizer skipped this step (afft_sgd_fused_t.ok): the average does not move
  f32x4* __restrict__ e4 = (f32x4*)ema;
  const f32x4* __restrict__ p4 = (const f32x4*)p;
  const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + (kStreamUnroll - 1) * stride < n4; i += kStreamUnroll * stride) {
    f32x4 ev[kStreamUnroll], pv[kStreamUnroll];
#pragma unroll
    for (int r = 0; r < kStreamUnroll; ++r) { ev[r] = e4[i + r * stride]; pv[r] = p4[i + r * stride]; }
#pragma unroll
    for (int r = 0; r < kStreamUnroll; ++r) e4[i + r * stride] = ema_update4(ev[r], pv[r], w);
  }
  for (; i < n4; i += stride) e4[i] = ema_update4(e4[i], p4[i], w);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t j = (n4 << 2) + threadIdx.x;
    ema[j] = ema_update(ema[j], p[j], w);
  }
}

// any 4-byte aligned bases: element accesses
__global__ __launch_bounds__(256) void ema_elem_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n, float w,
                                                       const float* __restrict__ ok) {
  if (ok && *ok == 0.f) return;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) ema[i] = ema_update(ema[i], p[i], w);
}

// the same two loops for the exchange: a bit copy each way (unsigned words, so that no NaN payload passes through a float move)
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
__global__ __launch_bounds__(256) void swap_kernel(unsigned* __restrict__ a, unsigned* __restrict__ b, int64_t n) {
  u32x4* __restrict__ a4 = (u32x4*)a;
  u32x4* __restrict__ b4 = (u32x4*)b;
  const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + (kStreamUnroll - 1) * stride < n4; i += kStreamUnroll * stride) {
    u32x4 av[kStreamUnroll], bv[kStreamUnroll];
#pragma unroll
    for (int r = 0; r < kStreamUnroll; ++r) { av[r] = a4[i + r * stride]; bv[r] = b4[i + r * stride]; }
#pragma unroll
    for (int r = 0; r < kStreamUnroll; ++r) { a4[i + r * stride] = bv[r]; b4[i + r * stride] = av[r]; }
  }
  for (; i < n4; i += stride) { const u32x4 av = a4[i], bv = b4[i]; a4[i] = bv; b4[i] = av; }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t j = (n4 << 2) + threadIdx.x;
    const unsigned av = a[j], bv = b[j];
    a[j] = bv; b[j] = av;
  }
}
__global__ __launch_bounds__(256) void swap_elem_kernel(unsigned* __restrict__ a, unsigned* __restrict__ b, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const unsigned av = a[i], bv = b[i];
    a[i] = bv; b[i] = av;
  }
}

// the grid cap of the flat updates (afft_sgd_nesterov2: one block per CU; AFFT_SGD_BLOCKS overrides), over `work` thread-iterations
int flat_update_blocks(int64_t work) {
  static const int64_t max_blocks = [] {
    const char* e = getenv("AFFT_SGD_BLOCKS");
    const long val = e ? atol(e) : 0;
    return (int64_t)(val > 0 ? val : 256);
  }();
  int64_t blocks = (work + 255) / 256;
  if (blocks < 1) blocks = 1;
  return (int)(blocks > max_blocks ? max_blocks : blocks);
}

}  // namespace

extern "C" int afft_adam(float* p, const void* g, int32_t g_dtype, float* m, float* v, void* p_bf16, void* p_f16, void* p_f8,
                         int64_t n, float lr, float beta1, float beta2, float eps, float wd, float gscale, const float* gscale_dev,
                         const float* step_dev, int32_t flags, const float* ok, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(p && g && m && v && step_dev, "adam: null pointer");
  AFFT_CHECK(((uintptr_t)p & 15) == 0 && ((uintptr_t)g & 15) == 0 && ((uintptr_t)m & 15) == 0 && ((uintptr_t)v & 15) == 0,
             "adam: buffers must be 16-byte aligned");
  AFFT_CHECK(g_dtype == AFFT_F32 || g_dtype == AFFT_BF16, "adam: bad gradient dtype");
  AFFT_CHECK(n >= 0, "adam: negative length");
  if (n == 0) return 0;
  // the grid cap of the SGD update (one block per CU, so the update beside the backward GEMMs keeps few CUs)
  hipLaunchKernelGGL(adam_kernel, dim3(flat_update_blocks((n + 3) / 4)), dim3(256), 0, stream, p, g, g_dtype, m, v, (bf16_t*)p_bf16, (bf16_t*)p_f16,
                     (unsigned char*)p_f8, n, lr, beta1, beta2, eps, wd, gscale, gscale_dev, step_dev, flags, ok);
  AFFT_LAUNCH_CHECK();
  return 0;
}

extern "C" int afft_adam_runs(float* p, const float* g, float* m, float* v, void* p_bf16, void* p_f16, void* p_f8,
                              const int64_t* runs, int32_t nruns, float lr, float beta1, float beta2, float eps, float wd,
                              float gscale, const float* step_dev, int32_t flags, const float* ok, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(p && g && m && v && step_dev && (runs || nruns == 0), "adam_runs: null pointer");
  if (nruns <= 0) return 0;
  hipLaunchKernelGGL(adam_runs_kernel, dim3(nruns), dim3(256), 0, stream, p, g, m, v, (bf16_t*)p_bf16, (bf16_t*)p_f16,
                     (unsigned char*)p_f8, runs, lr, beta1, beta2, eps, wd, gscale, step_dev, flags, ok);
  AFFT_LAUNCH_CHECK();
  return 0;
}

extern "C" int afft_ema(float* ema, const float* p, int64_t n, float w, const float* ok, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(n >= 0, "ema: negative length");
  AFFT_CHECK(w >= 0.f && w <= 1.f, "ema: w must lie in [0, 1] (got %g)", (double)w);      // a NaN fails both comparisons
  AFFT_CHECK(n == 0 || (ema && p), "ema: null pointer");
  AFFT_CHECK((((uintptr_t)ema | (uintptr_t)p) & 3) == 0, "ema: buffers must be 4-byte aligned");
  if (n == 0 || w == 0.f) return 0;      // w = 0 (decay 1): the average stays as it is, bit for bit
  AfftKernelScope ktrace(AFFT_K_EMA, (int)(n > INT_MAX ? INT_MAX : n), 1, 12 * n, 0, stream);
  if ((((uintptr_t)ema | (uintptr_t)p) & 15) == 0)
    hipLaunchKernelGGL(ema_kernel, dim3(flat_update_blocks(n >> 2)), dim3(256), 0, stream, ema, p, n, w, ok);
  else
    hipLaunchKernelGGL(ema_elem_kernel, dim3(flat_update_blocks(n)), dim3(256), 0, stream, ema, p, n, w, ok);
  AFFT_LAUNCH_CHECK();
  return 0;
}

extern "C" int afft_swap_f32(float* a, float* b, int64_t n, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(n >= 0, "swap_f32: negative length");
  AFFT_CHECK(n == 0 || (a && b), "swap_f32: null pointer");
  AFFT_CHECK((((uintptr_t)a | (uintptr_t)b) & 3) == 0, "swap_f32: buffers must be 4-byte aligned");
  if (n == 0) return 0;
  AFFT_CHECK((uintptr_t)a + 4 * (uintptr_t)n <= (uintptr_t)b || (uintptr_t)b + 4 * (uintptr_t)n <= (uintptr_t)a,
             "swap_f32: the buffers overlap");
  AfftKernelScope ktrace(AFFT_K_SWAP_F32, (int)(n > INT_MAX ? INT_MAX : n), 1, 16 * n, 0, stream);
  if ((((uintptr_t)a | (uintptr_t)b) & 15) == 0)
    hipLaunchKernelGGL(swap_kernel, dim3(flat_update_blocks(n >> 2)), dim3(256), 0, stream, (unsigned*)a, (unsigned*)b, n);
  else
    hipLaunchKernelGGL(swap_elem_kernel, dim3(flat_update_blocks(n)), dim3(256), 0, stream, (unsigned*)a, (unsigned*)b, n);
  AFFT_LAUNCH_CHECK();
  return 0;
}
