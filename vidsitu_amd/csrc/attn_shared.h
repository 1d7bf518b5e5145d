// What the whole-sequence attention kernels share: the exact-fp32 matrix instruction with its LDS staging and the
// dropout draw of the matrix-unit kernels (roberta_ops.hip, attn_tiled.hip), and the LDS budget of the resident
// kernels (roberta_ops.hip, gpt2_ops.hip, attn_cross.hip) -- each formula once, for the launchers' own checks and for
// vs_attn_resident_fits / vs_attn_cross_fits.
#pragma once
#include "common.h"
#include "dropout_rng.h"

#define AP_QT 64
// dynamic LDS a block may ask for: the 160 KiB of a CU less 1 KiB for the compiler's own static LDS (the block-wide
// "or" below keeps its flag there; with the full 160 KiB hipFuncSetAttribute refuses the kernel)
#define AP_LDS_MAX (159 * 1024)
// queries (keys) per block of the resident causal kernels
#define AC_QC 16
#define AC_LDS_MAX (160 * 1024)

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// rows 0 .. L-1 of a [L][DH] slice (row pitch `stride` floats) into LDS [Lp][DH + 4]; rows L .. Lp-1 are zero
template <int DH>
__device__ __forceinline__ void ap_stage(float* dst, const float* src, long long stride, int L, int Lp) {
  constexpr int LD = DH + 4, V4 = DH / 4;
  for (int i = threadIdx.x; i < Lp * V4; i += 256) {
    const int j = i / V4, c = i - j * V4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < L) v = *(const float4*)(src + (long long)j * stride + c * 4);
    *(float4*)(dst + j * LD + c * 4) = v;
  }
}

// The additive mask without its rounding: -1e4 on a score leaves the sum with an ulp of 2^-10, and exp(s - 1e4 - max)
// is exactly zero (in fp64 too) beside any key that is not masked.  So: a sequence with at least one valid key gives
// its masked keys the score -inf (weight exactly 0); a sequence whose mask is all zero has the same -1e4 on every
// key, which the softmax does not see -- it runs unmasked.  Both equal the stated formula for |s| < 9e3.
// -> true when masked keys are to be dropped; every thread of the block must call it.
__device__ __forceinline__ bool ap_any_key_valid(const uint8_t* kmask, int r, int L) {
  int any = 0;
  if (kmask)
    for (int j = threadIdx.x; j < L; j += 256) any |= kmask[(long long)r * L + j];
  return __syncthreads_or(any) != 0;
}

// DROP (train-mode dropout on the probabilities, out_i = sum_j p_ij m_ij v_j with the row sum taken before the mask):
// element index of (r, h, i, j) = ((r * H + h) * L + i) * Lp4 + j with Lp4 = (L + 3) & ~3 -- the causal kernel's
// convention, not this kernel's 16-wide Lp -- so four consecutive keys of a query are one Philox block.  The softmax
// passes give a row's four lanes the columns c0, c0 + 4, ...; the mask passes give them whole blocks (columns 4b ..
// 4b + 3 for b = c0, c0 + 4, ...): one draw per four keys, and the plain kernel's summation order stays as it is.
// -> the four multipliers (0 or scale) of block b of the row whose first block is rowblk
__device__ __forceinline__ float4 ap_mask4(const DropArgs& dr, uint64_t seed, uint64_t step, uint64_t rowblk, int b) {
  const vs_philox_out w = vs_dropout_block(seed, step, dr.site, rowblk + (uint64_t)b);
  return make_float4(w.w[0] >= dr.thr ? dr.scale : 0.f, w.w[1] >= dr.thr ? dr.scale : 0.f,
                     w.w[2] >= dr.thr ? dr.scale : 0.f, w.w[3] >= dr.thr ? dr.scale : 0.f);
}

// ---- LDS of the resident kernels (bytes) ----
static inline int ap_lp(int L) { return (L + 15) / 16 * 16; }
static inline size_t ap_fwd_smem(int L, int dh) {
  const int Lp = ap_lp(L);
  return ((size_t)2 * Lp * (dh + 4) + 4 * 16 * (Lp + 4)) * sizeof(float);
}
static inline size_t ap_bwd_smem(int L, int dh) {
  const int Lp = ap_lp(L);
  return ((size_t)2 * Lp * (dh + 4) + 8 * 16 * (Lp + 4)) * sizeof(float);
}
static inline bool ap_dh_ok(int dh) { return dh == 16 || dh == 32 || dh == 64 || dh == 128; }

// the cross-attention kernels (attn_cross.hip): K and V of the SOURCE are what is resident, so the forward and the
// backward's query launch take ap_fwd_smem(S, dh) / ap_bwd_smem(S, dh) whatever L; the backward's key launch passes Q
// and dO through LDS AP_QT queries at a time
static inline size_t ax_bwd_kv_smem(int dh) { return (size_t)2 * AP_QT * (dh + 4) * sizeof(float); }
// keys of the cached decode step: four waves' score strips of S floats stay inside the default 64 KiB
#define AX_DEC_SMAX 2048

// the causal kernels: K and V of the head at pitch dh + 1, per-wave probability rows, the chunk's q / dO rows
static inline size_t ac_fwd_smem(int L, int dh) {
  const size_t l = (size_t)L, d = (size_t)dh;
  return (2 * l * (d + 1) + 4 * l + 4 * d) * sizeof(float);
}
static inline size_t ac_bwd_q_smem(int L, int dh) {
  const size_t l = (size_t)L, d = (size_t)dh;
  return ((2 * l + 2 * AC_QC) * (d + 1) + 8 * l) * sizeof(float);
}
static inline size_t ac_bwd_kv_smem(int L, int dh) {
  const size_t l = (size_t)L, d = (size_t)dh;
  return (2 * l * (d + 1) + 2 * l * AC_QC) * sizeof(float);
}
