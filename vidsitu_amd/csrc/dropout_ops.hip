// Train-mode dropout from the counter generator of dropout_rng.h: the state tick, the elementwise
// residual-site kernel and the host-side mask.  The attention and embedding sites live beside the kernels they
// extend (gpt2_ops.hip); nothing here knows a model.
#include <math.h>

#include "common.h"
#include "dropout_rng.h"

// p -> (thr, scale) of the contract, in double, once, on the host.
extern "C" int vs_dropout_threshold(double p, uint32_t* thr, float* scale) {
  VS_CHECK_ARG(thr && scale, "bad args");
  VS_CHECK_ARG(p >= 0.0 && p < 1.0, "dropout probability must satisfy 0 <= p < 1");
  const double t = floor(p * 4294967296.0 + 0.5);
  *thr = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
  *scale = (float)(1.0 / (1.0 - p));
  return VS_OK;
}

extern "C" int vs_dropout_mask_host(uint64_t seed, uint64_t step, uint32_t site, uint64_t e0, int64_t n,
                                    uint32_t thr, uint8_t* keep) {
  VS_CHECK_ARG(keep && n > 0, "bad args");
  for (int64_t i = 0; i < n; ++i) keep[i] = (uint8_t)vs_dropout_keep(seed, step, site, e0 + (uint64_t)i, thr);
  return VS_OK;
}

// snap = state; state.step += 1.  The only writer of `state`; captured with the step, so every replay of a graph
// draws the masks of its own step while the kernels of one step all read the same snapshot.
__global__ void dropout_tick_kernel(int64_t* state, int64_t* snap) {
  const int64_t seed = state[0], step = state[1];
  snap[0] = seed;
  snap[1] = step;
  state[1] = step + 1;
}

extern "C" int vs_dropout_tick(int64_t* state, int64_t* snap, void* stream) {
  VS_CHECK_ARG(state && snap && state != snap, "bad args");
  hipLaunchKernelGGL(dropout_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, snap);
  VS_CHECK_LAUNCH();
  return VS_OK;
}

// out = res + m * x, four elements (one Philox block, 16-byte accesses) per thread; n4 = n / 4 blocks.
template <bool RES>
__global__ __launch_bounds__(256) void dropout_add_vec_kernel(const float4* __restrict__ x,
                                                              const float4* __restrict__ res,
                                                              float4* __restrict__ out, long long n4,
                                                              const int64_t* __restrict__ snap, uint32_t site,
                                                              uint32_t thr, float scale) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= n4) return;
  const vs_philox_out o = vs_dropout_block((uint64_t)snap[0], (uint64_t)snap[1], site, (uint64_t)b);
  const float4 v = x[b];
  float4 y;
  y.x = o.w[0] >= thr ? v.x * scale : 0.f;
  y.y = o.w[1] >= thr ? v.y * scale : 0.f;
  y.z = o.w[2] >= thr ? v.z * scale : 0.f;
  y.w = o.w[3] >= thr ? v.w * scale : 0.f;
  if (RES) {
    const float4 r = res[b];
    y.x += r.x;
    y.y += r.y;
    y.z += r.z;
    y.w += r.w;
  }
  out[b] = y;
}

// The same, one element per thread: n % 4 != 0 or a pointer off the 16-byte grid.
template <bool RES>
__global__ __launch_bounds__(256) void dropout_add_scalar_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ res,
                                                                 float* __restrict__ out, long long n,
                                                                 const int64_t* __restrict__ snap, uint32_t site,
                                                                 uint32_t thr, float scale) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const vs_philox_out o = vs_dropout_block((uint64_t)snap[0], (uint64_t)snap[1], site, (uint64_t)e >> 2);
  const int k = (int)(e & 3);
  const uint32_t w = k == 0 ? o.w[0] : k == 1 ? o.w[1] : k == 2 ? o.w[2] : o.w[3];
  float y = w >= thr ? x[e] * scale : 0.f;
  if (RES) y += res[e];
  out[e] = y;
}

extern "C" int vs_dropout_add_f32(const float* x, const float* res, float* out, int64_t n, const int64_t* snap,
                                  uint32_t site, uint32_t thr, float scale, void* stream) {
  VS_CHECK_ARG(x && out && snap && n > 0, "bad args");
  VS_CHECK_ARG(n <= ((int64_t)1 << 38), "more elements than one launch's grid covers");
  const bool vec = n % 4 == 0 && (((uintptr_t)x | (uintptr_t)out | (uintptr_t)res) & 15) == 0;
  const long long work = vec ? n / 4 : n;
  const dim3 grid((unsigned)((work + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  if (vec) {
    if (res)
      hipLaunchKernelGGL(dropout_add_vec_kernel<true>, grid, dim3(256), 0, st, (const float4*)x,
                         (const float4*)res, (float4*)out, work, snap, site, thr, scale);
    else
      hipLaunchKernelGGL(dropout_add_vec_kernel<false>, grid, dim3(256), 0, st, (const float4*)x,
                         (const float4*)nullptr, (float4*)out, work, snap, site, thr, scale);
  } else {
    if (res)
      hipLaunchKernelGGL(dropout_add_scalar_kernel<true>, grid, dim3(256), 0, st, x, res, out, work, snap, site,
                         thr, scale);
    else
      hipLaunchKernelGGL(dropout_add_scalar_kernel<false>, grid, dim3(256), 0, st, x, (const float*)nullptr, out,
                         work, snap, site, thr, scale);
  }
  VS_CHECK_LAUNCH();
  return VS_OK;
}
