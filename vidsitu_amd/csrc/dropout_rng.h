// Counter-based dropout masks: one Philox4x32-10 shared by host and device code.  A mask is a pure function of
// (seed, step, site, element index), so the kernel that applies it and the kernel that differentiates through it
// both compute it and nothing is stored between them.
//
// Contract (restated by tests/dropout_ref.py):
//   key     = (seed low 32 bits, seed high 32 bits)
//   counter = (b low 32, b high 32, site, step low 32)  with b = e >> 2; element e takes word e & 3 of that block
//   keep    = word >= thr,  thr = (uint32) floor(p * 2^32 + 0.5)  (thr = 0 keeps everything)
//   kept elements are multiplied by scale = 1 / (1 - p)
// What an element index means is the caller's business (a flat row-major index for elementwise sites, a padded-pitch
// index for attention probabilities); this header knows no model.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VS_RNG_HD __host__ __device__ __forceinline__
#else
#define VS_RNG_HD static inline
#endif

struct vs_philox_out {
  uint32_t w[4];
};

VS_RNG_HD uint32_t vs_mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers 0xD2511F53 /
// 0xCD9E8D57, Weyl key increments 0x9E3779B9 / 0xBB67AE85, ten rounds.
VS_RNG_HD vs_philox_out vs_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                         uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = vs_mulhi32(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = vs_mulhi32(M1, c2), lo1 = M1 * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  vs_philox_out o;
  o.w[0] = c0;
  o.w[1] = c1;
  o.w[2] = c2;
  o.w[3] = c3;
  return o;
}

// The four words of dropout block b (elements 4b .. 4b+3) of one site at one step.
VS_RNG_HD vs_philox_out vs_dropout_block(uint64_t seed, uint64_t step, uint32_t site, uint64_t b) {
  return vs_philox4x32_10((uint32_t)b, (uint32_t)(b >> 32), site, (uint32_t)step, (uint32_t)seed,
                          (uint32_t)(seed >> 32));
}

// 1 when element e is kept.
VS_RNG_HD int vs_dropout_keep(uint64_t seed, uint64_t step, uint32_t site, uint64_t e, uint32_t thr) {
  const vs_philox_out o = vs_dropout_block(seed, step, site, e >> 2);
  return o.w[e & 3] >= thr;
}

// What a kernel with a dropout site takes: the step's snapshot and the site's number, threshold and scale.
struct DropArgs {
  const int64_t* snap;  // [seed, step] of this step (vs_dropout_tick)
  uint32_t site, thr;
  float scale;
};
