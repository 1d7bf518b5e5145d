// Key-tiled self-attention (fp32 on v_mfma_f32_16x16x4_f32), forward and backward, for the sequences the LDS-resident
// kernels (roberta_ops.hip: padding mask; gpt2_ops.hip: causal) cannot hold: K and V pass through LDS one tile of 64
// keys at a time under an online softmax, so a block's LDS is fixed per head width and no L x L matrix is ever stored.
// One kernel text per launch, templated on <DH, CAUSAL, DROP>; operand maps, the dh + 4 pitch, the staging and the
// dropout draw are those of roberta_ops.hip (attn_shared.h).
//
// Masking rules (j = key, i = query; columns j >= L have weight exactly 0 and never enter a maximum):
//   pad    (CAUSAL = false): ap_any_key_valid's rule -- a sequence with a valid key gives its masked keys the score -inf,
//          a sequence whose mask is all zero runs unmasked.  A key tile with no valid key is skipped.
//   causal (CAUSAL = true):  attn_causal_kernel's arithmetic, literally: s = dot * scale where j <= i, else -1e4f; then
//          s += -1e4f where the key is masked; softmax over all L keys.  A (64 queries, 64 keys) pair is skipped only
//          where that is exact: every query before every key, and every query at or after the sequence's first valid
//          position (it then has a visible unmasked key, beside which exp(-1e4 - max) is exactly 0).  Queries in front
//          of left padding give weight to future keys; their pairs are computed literally, in launch B as well.
// Dropout: element (r, h, i, j) = ((r*H + h)*L + i) * Lp4 + j, Lp4 = (L + 3) & ~3; the tile width is a multiple of 4,
//   so every draw is a whole Philox block of one query's four consecutive keys -- the mask is a function of the
//   element alone, whichever family serves the forward or the backward of a step.
// Every output element has one owner and a fixed summation order: no atomics, two runs agree bit for bit.
#include <math.h>

#include "attn_shared.h"
#include "common.h"

#define AT_KT 64            // keys per tile (query tiles in launch B)
#define AT_LS (AT_KT + 4)   // pitch of a wave's [16][AT_KT] strip
#define AT_L_MAX (65535 * AP_QT)  // gridDim.y

// -> the sequence's first valid position: 0 without a mask, L when the mask row is all zero.  Every thread calls it.
__device__ __forceinline__ int at_first_valid(const uint8_t* kmask, int r, int L) {
  __shared__ int red[4];
  if (!kmask) return 0;
  int fv = L;
  for (int j = threadIdx.x; j < L; j += 256)
    if (kmask[(long long)r * L + j]) fv = min(fv, j);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) fv = min(fv, __shfl_xor(fv, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = fv;
  __syncthreads();
  return min(min(red[0], red[1]), min(red[2], red[3]));
}

// Block-uniform: does the pair (queries q0 .. q0 + 63, keys j0 .. j0 + 63) contribute nothing, exactly?
template <bool CAUSAL>
__device__ __forceinline__ bool at_skip(const uint8_t* km, bool masked, int fv, int q0, int j0, int L) {
  if (CAUSAL) return j0 > min(L, q0 + AP_QT) - 1 && q0 >= fv;
  if (!masked) return false;
  int any = 0;  // pad: a tile without a valid key
  if (threadIdx.x < AT_KT && j0 + (int)threadIdx.x < L) any = km[j0 + threadIdx.x];
  return __syncthreads_or(any) == 0;
}

// The wave's raw score tile [16 queries][64 keys] into its strip, masked by the rule.  km: the sequence's mask row.
template <int DH, bool CAUSAL>
__device__ __forceinline__ void at_scores(const float* qf, const float* Ks, float* Sw, const uint8_t* km, bool masked,
                                          int i0w, int j0, int L, float scale, int lr, int lq) {
  constexpr int LD = DH + 4, KS = DH / 4;
#pragma unroll
  for (int jt = 0; jt < AT_KT / 16; ++jt) {
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};  // even / odd k steps: two independent chains
    const float* kp = Ks + (jt * 16 + lr) * LD + lq;
#pragma unroll
    for (int k = 0; k < KS; k += 2) {
      a0 = mfma4(qf[k], kp[k * 4], a0);
      a1 = mfma4(qf[k + 1], kp[k * 4 + 4], a1);
    }
    const int j = j0 + jt * 16 + lr;
    const bool off = km && j < L && !km[j];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float s = (a0[g] + a1[g]) * scale;
      if (CAUSAL) {
        if (j > i0w + lq * 4 + g) s = -1e4f;
        if (off) s += -1e4f;
      } else if (masked && off) {
        s = -INFINITY;
      }
      if (j >= L) s = -INFINITY;
      Sw[(lq * 4 + g) * AT_LS + jt * 16 + lr] = s;
    }
  }
}

// dP = dO V^T of the same tile into the second strip
template <int DH>
__device__ __forceinline__ void at_dp(const float* of, const float* Vs, float* Dw, int lr, int lq) {
  constexpr int LD = DH + 4, KS = DH / 4;
#pragma unroll
  for (int jt = 0; jt < AT_KT / 16; ++jt) {
    f32x4 b0 = {0.f, 0.f, 0.f, 0.f};
    const float* vp = Vs + (jt * 16 + lr) * LD + lq;
#pragma unroll
    for (int k = 0; k < KS; ++k) b0 = mfma4(of[k], vp[k * 4], b0);
#pragma unroll
    for (int g = 0; g < 4; ++g) Dw[(lq * 4 + g) * AT_LS + jt * 16 + lr] = b0[g];
  }
}

// v o m.  The product is rounded on its own (this file is compiled without multiply-add contraction, see the Makefile):
// m o dP meets D_i = sum_j p_ij (m o dP)_ij in a subtraction, and contracted into it the product would be the
// unrounded one -- a row with one valid key has dS = p (m dP - D) = 0 exactly, and must have it in both launches
__device__ __forceinline__ float4 at_mask4(float4 v, float4 m) {
  return make_float4(v.x * m.x, v.y * m.y, v.z * m.z, v.w * m.w);
}
__device__ __forceinline__ float at_max4(float4 v) { return fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)); }
__device__ __forceinline__ float4 at_exp4(float4 v, float m) {
  return make_float4(expf(v.x - m), expf(v.y - m), expf(v.z - m), expf(v.w - m));
}

// ----------------------------------------------------------------------------
// Forward.  One block per (sequence, head, 64 queries), four waves of 16 queries with their Q fragments in registers;
// per key tile: scores into the wave's strip, four lanes per row update the running maximum m and sum l (the lanes of
// a row take the blocks of four columns c0, c0 + 4, ...), the O accumulator [16][DH] is rescaled by exp(m_old - m_new)
// and takes e V on the matrix unit; out = O / l.  Under DROP e is masked after the row sum took it.
// LDS: 2 * 64 * (DH + 4) + 4 * 16 * 68 floats = 51 KiB at DH = 64 (three blocks per CU), 83 KiB at DH = 128.
// ----------------------------------------------------------------------------
template <int DH, bool CAUSAL, bool DROP>
__global__ __launch_bounds__(256) void attn_tiled_fwd_kernel(const float* __restrict__ qkv,
                                                             const uint8_t* __restrict__ kmask,
                                                             float* __restrict__ out, int L, int H, DropArgs dr) {
  extern __shared__ float sm[];
  constexpr int LD = DH + 4, KS = DH / 4, CT = DH / 16;
  const int D = H * DH;
  const int r = blockIdx.x / H, h = blockIdx.x % H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  float* Ks = sm;
  float* Vs = Ks + AT_KT * LD;
  float* Sw = Vs + AT_KT * LD + wave * 16 * AT_LS;
  const float* base = qkv + (long long)r * L * 3 * D + h * DH;
  const uint8_t* km = kmask ? kmask + (long long)r * L : nullptr;
  const int q0 = blockIdx.y * AP_QT, i0 = q0 + wave * 16;
  const bool active = i0 < L;  // wave-uniform
  float qf[KS];
  {
    const int i = i0 + lr;
#pragma unroll
    for (int k = 0; k < KS; ++k) qf[k] = i < L ? base[(long long)i * 3 * D + k * 4 + lq] : 0.f;
  }
  const int fv = at_first_valid(kmask, r, L);
  const bool masked = kmask && fv < L;
  const float scale = 1.0f / sqrtf((float)DH);
  const int c0 = lane & 3, irow = i0 + (lane >> 2);  // softmax layout: row lane >> 2, blocks c0, c0 + 4, c0 + 8, c0 + 12
  float* row = Sw + (lane >> 2) * AT_LS;
  uint64_t seed = 0, step = 0, rowblk = 0;
  if (DROP) {
    seed = (uint64_t)dr.snap[0];
    step = (uint64_t)dr.snap[1];
    rowblk = ((uint64_t)blockIdx.x * L + (irow < L ? irow : 0)) * (uint64_t)((L + 3) >> 2);
  }
  float m = -INFINITY, l = 0.f;
  f32x4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int j0 = 0; j0 < L; j0 += AT_KT) {
    if (at_skip<CAUSAL>(km, masked, fv, q0, j0, L)) continue;
    __syncthreads();  // the tile before this one is used up
    ap_stage<DH>(Ks, base + D + (long long)j0 * 3 * D, 3LL * D, min(AT_KT, L - j0), AT_KT);
    ap_stage<DH>(Vs, base + 2 * D + (long long)j0 * 3 * D, 3LL * D, min(AT_KT, L - j0), AT_KT);
    __syncthreads();
    if (!active) continue;
    at_scores<DH, CAUSAL>(qf, Ks, Sw, km, masked, i0, j0, L, scale, lr, lq);
    __builtin_amdgcn_wave_barrier();  // the strip is the wave's own: its LDS traffic is in program order
    float4 v[4];
    float mt = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      v[t] = *(const float4*)(row + (c0 + 4 * t) * 4);
      mt = fmaxf(mt, at_max4(v[t]));
    }
    mt = fmaxf(mt, __shfl_xor(mt, 1, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 2, 64));
    const float mn = fmaxf(m, mt);       // finite: a tile that is not skipped has a key of finite score
    const float alpha = expf(m - mn);    // 0 on the first tile (m = -inf)
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float4 e = at_exp4(v[t], mn);
      sum += (e.x + e.y) + (e.z + e.w);
      if (DROP) {
        const int b = (j0 >> 2) + c0 + 4 * t;
        if (irow < L && b * 4 < L) {  // past L: e is 0 and stays 0
          const float4 mk = ap_mask4(dr, seed, step, rowblk, b);
          e = at_mask4(e, mk);
        }
      }
      *(float4*)(row + (c0 + 4 * t) * 4) = e;
    }
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    l = l * alpha + sum;
    m = mn;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float ar = __shfl(alpha, (lq * 4 + g) * 4, 64);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[ct][g] *= ar;
    }
#pragma unroll 4
    for (int k = 0; k < AT_KT / 4; ++k) {
      const float a = Sw[lr * AT_LS + k * 4 + lq];
      const float* vp = Vs + (k * 4 + lq) * LD + lr;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[ct] = mfma4(a, vp[ct * 16], acc[ct]);
    }
  }
  if (active) {
    const float inv = 1.0f / l;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int rw = lq * 4 + g, i = i0 + rw;
      const float rinv = __shfl(inv, rw * 4, 64);
      if (i < L) {
        float* o = out + ((long long)r * L + i) * D + h * DH + lr;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) o[ct * 16] = acc[ct][g] * rinv;
      }
    }
  }
}

// ----------------------------------------------------------------------------
// Backward in two launches, p re-derived from q, k and the masks (the forward stores nothing).
// Launch A (64 queries per block, 16 per wave) sweeps the key tiles twice:
//   sweep 1: s and dP = dO V^T per tile; running m, l and sum_j e_ij dP_ij under the same rescaling -> the row
//            statistics (m, 1/l) and D_i = sum_j p_ij dP_ij (undropped p, masked dP under DROP), written to the scratch
//            [R*H][3][L];
//   sweep 2: s and dP again, p = exp(s - m) / l, dS = p (dP - D) (no dS for a future key under CAUSAL: its score is a
//            constant), dQ = scale * dS K accumulated on the matrix unit.
//   Two sweeps, not the one-sweep split dQ = scale (sum p dP k - D sum p k): the split subtracts two sums of the size
//   of |dP| |k| to get one of the size of |dP - D| |k| and loses digits where the softmax is flat; this form has the
//   resident kernel's rounding.
// Launch B (64 keys per block, 16 per wave, K and V fragments in registers) sweeps the query tiles: s^T = K Q^T and
//   dP^T = V dO^T per tile, p and dS from the scratch rows in registers (one Philox block per lane and 16 x 16 tile:
//   a lane's four accumulator rows are four consecutive keys of one query), through the wave's strips as the A operand
//   of dV = (p o m)^T dO and dK = scale * dS^T Q.
// LDS of either launch: 2 * 64 * (DH + 4) + 8 * 16 * 68 floats = 68 KiB at DH = 64 (two blocks per CU).
// ----------------------------------------------------------------------------
template <int DH, bool CAUSAL, bool DROP>
__global__ __launch_bounds__(256) void attn_tiled_bwd_q_kernel(const float* __restrict__ qkv,
                                                               const uint8_t* __restrict__ kmask,
                                                               const float* __restrict__ dout,
                                                               float* __restrict__ dqkv, float* __restrict__ scratch,
                                                               int L, int H, DropArgs dr) {
  extern __shared__ float sm[];
  constexpr int LD = DH + 4, KS = DH / 4, CT = DH / 16;
  const int D = H * DH;
  const int r = blockIdx.x / H, h = blockIdx.x % H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  float* Ks = sm;
  float* Vs = Ks + AT_KT * LD;
  float* Pw = Vs + AT_KT * LD + wave * 32 * AT_LS;  // s, then e / p
  float* Dw = Pw + 16 * AT_LS;                      // dP, then dS
  const float* base = qkv + (long long)r * L * 3 * D + h * DH;
  const float* dob = dout + (long long)r * L * D + h * DH;
  const uint8_t* km = kmask ? kmask + (long long)r * L : nullptr;
  float* stat = scratch + (long long)blockIdx.x * 3 * L;  // m[L], 1/l[L], D[L]
  const int q0 = blockIdx.y * AP_QT, i0 = q0 + wave * 16;
  const bool active = i0 < L;
  float qf[KS], of[KS];
  {
    const int i = i0 + lr;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      qf[k] = i < L ? base[(long long)i * 3 * D + k * 4 + lq] : 0.f;
      of[k] = i < L ? dob[(long long)i * D + k * 4 + lq] : 0.f;
    }
  }
  const int fv = at_first_valid(kmask, r, L);
  const bool masked = kmask && fv < L;
  const float scale = 1.0f / sqrtf((float)DH);
  const int c0 = lane & 3, irow = i0 + (lane >> 2);
  float* row = Pw + (lane >> 2) * AT_LS;
  float* drow = Dw + (lane >> 2) * AT_LS;
  uint64_t seed = 0, step = 0, rowblk = 0;
  if (DROP) {
    seed = (uint64_t)dr.snap[0];
    step = (uint64_t)dr.snap[1];
    rowblk = ((uint64_t)blockIdx.x * L + (irow < L ? irow : 0)) * (uint64_t)((L + 3) >> 2);
  }
  float m = -INFINITY, l = 0.f, dacc = 0.f;
  for (int j0 = 0; j0 < L; j0 += AT_KT) {  // sweep 1
    if (at_skip<CAUSAL>(km, masked, fv, q0, j0, L)) continue;
    __syncthreads();
    ap_stage<DH>(Ks, base + D + (long long)j0 * 3 * D, 3LL * D, min(AT_KT, L - j0), AT_KT);
    ap_stage<DH>(Vs, base + 2 * D + (long long)j0 * 3 * D, 3LL * D, min(AT_KT, L - j0), AT_KT);
    __syncthreads();
    if (!active) continue;
    at_scores<DH, CAUSAL>(qf, Ks, Pw, km, masked, i0, j0, L, scale, lr, lq);
    at_dp<DH>(of, Vs, Dw, lr, lq);
    __builtin_amdgcn_wave_barrier();
    float4 v[4];
    float mt = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      v[t] = *(const float4*)(row + (c0 + 4 * t) * 4);
      mt = fmaxf(mt, at_max4(v[t]));
    }
    mt = fmaxf(mt, __shfl_xor(mt, 1, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 2, 64));
    const float mn = fmaxf(m, mt);
    const float alpha = expf(m - mn);
    float sum = 0.f, dsum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float4 e = at_exp4(v[t], mn);
      float4 g = *(const float4*)(drow + (c0 + 4 * t) * 4);  // 0 past L (the V rows there are zero)
      sum += (e.x + e.y) + (e.z + e.w);
      if (DROP) {
        const int b = (j0 >> 2) + c0 + 4 * t;
        if (irow < L && b * 4 < L) {
          const float4 mk = ap_mask4(dr, seed, step, rowblk, b);
          g = at_mask4(g, mk);
        }
      }
      dsum += (e.x * g.x + e.y * g.y) + (e.z * g.z + e.w * g.w);
    }
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    dsum += __shfl_xor(dsum, 1, 64);
    dsum += __shfl_xor(dsum, 2, 64);
    l = l * alpha + sum;
    dacc = dacc * alpha + dsum;
    m = mn;
  }
  const float linv = 1.0f / l, dd = dacc * linv;
  if (active && c0 == 0 && irow < L) {
    stat[irow] = m;
    stat[L + irow] = linv;
    stat[2 * L + irow] = dd;
  }
  f32x4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int j0 = 0; j0 < L; j0 += AT_KT) {  // sweep 2
    if (at_skip<CAUSAL>(km, masked, fv, q0, j0, L)) continue;
    __syncthreads();
    ap_stage<DH>(Ks, base + D + (long long)j0 * 3 * D, 3LL * D, min(AT_KT, L - j0), AT_KT);
    ap_stage<DH>(Vs, base + 2 * D + (long long)j0 * 3 * D, 3LL * D, min(AT_KT, L - j0), AT_KT);
    __syncthreads();
    if (!active) continue;
    at_scores<DH, CAUSAL>(qf, Ks, Pw, km, masked, i0, j0, L, scale, lr, lq);
    at_dp<DH>(of, Vs, Dw, lr, lq);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = j0 + (c0 + 4 * t) * 4;
      const float4 e = at_exp4(*(const float4*)(row + (c0 + 4 * t) * 4), m);
      float4 g = *(const float4*)(drow + (c0 + 4 * t) * 4);
      if (DROP) {
        if (irow < L && j < L) {
          const float4 mk = ap_mask4(dr, seed, step, rowblk, j >> 2);
          g = at_mask4(g, mk);
        }
      }
      g.x = (e.x * linv) * (g.x - dd);
      g.y = (e.y * linv) * (g.y - dd);
      g.z = (e.z * linv) * (g.z - dd);
      g.w = (e.w * linv) * (g.w - dd);
      if (CAUSAL) {  // a future key's score is the constant -1e4: no gradient through it
        if (j > irow) g.x = 0.f;
        if (j + 1 > irow) g.y = 0.f;
        if (j + 2 > irow) g.z = 0.f;
        if (j + 3 > irow) g.w = 0.f;
      }
      *(float4*)(drow + (c0 + 4 * t) * 4) = g;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll 4
    for (int k = 0; k < AT_KT / 4; ++k) {
      const float a = Dw[lr * AT_LS + k * 4 + lq];
      const float* kp = Ks + (k * 4 + lq) * LD + lr;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[ct] = mfma4(a, kp[ct * 16], acc[ct]);
    }
  }
  if (active) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = i0 + lq * 4 + g;
      if (i < L) {
        float* o = dqkv + ((long long)r * L + i) * 3 * D + h * DH + lr;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) o[ct * 16] = acc[ct][g] * scale;
      }
    }
  }
}

template <int DH, bool CAUSAL, bool DROP>
__global__ __launch_bounds__(256) void attn_tiled_bwd_kv_kernel(const float* __restrict__ qkv,
                                                                const uint8_t* __restrict__ kmask,
                                                                const float* __restrict__ dout,
                                                                float* __restrict__ dqkv,
                                                                const float* __restrict__ scratch, int L, int H,
                                                                DropArgs dr) {
  extern __shared__ float sm[];
  constexpr int LD = DH + 4, KS = DH / 4, CT = DH / 16;
  const int D = H * DH;
  const int r = blockIdx.x / H, h = blockIdx.x % H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  float* Qs = sm;
  float* Os = Qs + AT_KT * LD;
  float* Pw = Os + AT_KT * LD + wave * 32 * AT_LS;  // (p o m)^T [16 keys][64 queries]
  float* Dw = Pw + 16 * AT_LS;                      // dS^T
  const float* base = qkv + (long long)r * L * 3 * D + h * DH;
  const float* dob = dout + (long long)r * L * D + h * DH;
  const uint8_t* km = kmask ? kmask + (long long)r * L : nullptr;
  const float* stat = scratch + (long long)blockIdx.x * 3 * L;
  const int jb0 = blockIdx.y * AP_QT, j0 = jb0 + wave * 16;
  const bool active = j0 < L;
  float kf[KS], vf[KS];
  {
    const int j = j0 + lr;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      kf[k] = j < L ? base[(long long)j * 3 * D + D + k * 4 + lq] : 0.f;
      vf[k] = j < L ? base[(long long)j * 3 * D + 2 * D + k * 4 + lq] : 0.f;
    }
  }
  const int fv = at_first_valid(kmask, r, L);
  const bool masked = kmask && fv < L;
  const float scale = 1.0f / sqrtf((float)DH);
  const int jg = j0 + lq * 4;  // the lane's four accumulator rows are the keys jg .. jg + 3
  bool off[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) off[g] = km && jg + g < L && !km[jg + g];
  uint64_t seed = 0, step = 0;
  if (DROP) {
    seed = (uint64_t)dr.snap[0];
    step = (uint64_t)dr.snap[1];
  }
  f32x4 av[CT], ak[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) av[ct] = ak[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < L; q0 += AT_KT) {
    if (CAUSAL && at_skip<true>(km, masked, fv, q0, jb0, L)) continue;  // (pad: a masked key has p = 0 in every tile)
    __syncthreads();
    ap_stage<DH>(Qs, base + (long long)q0 * 3 * D, 3LL * D, min(AT_KT, L - q0), AT_KT);
    ap_stage<DH>(Os, dob + (long long)q0 * D, (long long)D, min(AT_KT, L - q0), AT_KT);
    __syncthreads();
    if (!active) continue;
#pragma unroll
    for (int st = 0; st < AT_KT / 16; ++st) {
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f}, b0 = {0.f, 0.f, 0.f, 0.f};
      const float* qp = Qs + (st * 16 + lr) * LD + lq;
      const float* op = Os + (st * 16 + lr) * LD + lq;
#pragma unroll
      for (int k = 0; k < KS; k += 2) {  // the score in launch A's own order
        a0 = mfma4(kf[k], qp[k * 4], a0);
        a1 = mfma4(kf[k + 1], qp[k * 4 + 4], a1);
        b0 = mfma4(vf[k], op[k * 4], b0);
        b0 = mfma4(vf[k + 1], op[k * 4 + 4], b0);
      }
      const int i = q0 + st * 16 + lr;
      const bool live = i < L;  // a row past L: q = dO = 0 and the statistics read as 0 give p = dS = 0
      const float mi = live ? stat[i] : 0.f, li = live ? stat[L + i] : 0.f, di = live ? stat[2 * L + i] : 0.f;
      float4 mk = make_float4(1.f, 1.f, 1.f, 1.f);
      if (DROP && live && jg < L)
        mk = ap_mask4(dr, seed, step, ((uint64_t)blockIdx.x * L + i) * (uint64_t)((L + 3) >> 2), jg >> 2);
      const float mg[4] = {mk.x, mk.y, mk.z, mk.w};
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j = jg + g;
        float s = (a0[g] + a1[g]) * scale;
        if (CAUSAL) {
          if (j > i) s = -1e4f;
          if (off[g]) s += -1e4f;
        } else if (masked && off[g]) {
          s = -INFINITY;
        }
        if (j >= L) s = -INFINITY;
        const float p = expf(s - mi) * li;
        const float gd = DROP ? mg[g] * b0[g] : b0[g];  // (rounded on its own, as in launch A: at_mask4)
        float ds = p * (gd - di);
        if (CAUSAL && j > i) ds = 0.f;
        Pw[(lq * 4 + g) * AT_LS + st * 16 + lr] = DROP ? p * mg[g] : p;
        Dw[(lq * 4 + g) * AT_LS + st * 16 + lr] = ds;
      }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll 4
    for (int k = 0; k < AT_KT / 4; ++k) {
      const float ap = Pw[lr * AT_LS + k * 4 + lq];
      const float as = Dw[lr * AT_LS + k * 4 + lq];
      const float* op = Os + (k * 4 + lq) * LD + lr;
      const float* qp = Qs + (k * 4 + lq) * LD + lr;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        av[ct] = mfma4(ap, op[ct * 16], av[ct]);
        ak[ct] = mfma4(as, qp[ct * 16], ak[ct]);
      }
    }
    __builtin_amdgcn_wave_barrier();  // the strips are rewritten in the next tile
  }
  if (active) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int j = jg + g;
      if (j < L) {
        float* o = dqkv + ((long long)r * L + j) * 3 * D + D + h * DH + lr;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          o[ct * 16] = ak[ct][g] * scale;
          o[D + ct * 16] = av[ct][g];
        }
      }
    }
  }
}

// ---- host ----
static inline size_t at_fwd_smem(int dh) { return ((size_t)2 * AT_KT * (dh + 4) + 4 * 16 * AT_LS) * sizeof(float); }
static inline size_t at_bwd_smem(int dh) { return ((size_t)2 * AT_KT * (dh + 4) + 8 * 16 * AT_LS) * sizeof(float); }

static bool at_lds_attr(const void* kernel, size_t smem) {
  if (smem <= 64 * 1024) return true;  // (DH = 128 only)
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e == hipSuccess) return true;
  (void)hipGetLastError();
  vs_set_error("tiled attention kernel refused %zu bytes of dynamic LDS: %s", smem, hipGetErrorString(e));
  return false;
}

struct AtArgs {
  const float* qkv;
  const uint8_t* km;
  const float* dout;
  float* out;  // forward: out; backward: dqkv
  float* scratch;
  int R, L, H;
  DropArgs dr;
  hipStream_t st;
};

template <int DH, bool CAUSAL, bool DROP>
static int at_fwd_launch(const AtArgs& a) {
  static bool attr = false;  // (set on the eager call that has to precede a graph capture)
  if (!attr) {
    if (!at_lds_attr((const void*)attn_tiled_fwd_kernel<DH, CAUSAL, DROP>, at_fwd_smem(DH))) return VS_ERR_LAUNCH;
    attr = true;
  }
  hipLaunchKernelGGL((attn_tiled_fwd_kernel<DH, CAUSAL, DROP>), dim3(a.R * a.H, (a.L + AP_QT - 1) / AP_QT), dim3(256),
                     at_fwd_smem(DH), a.st, a.qkv, a.km, a.out, a.L, a.H, a.dr);
  return VS_OK;
}

template <int DH, bool CAUSAL, bool DROP>
static int at_bwd_launch(const AtArgs& a) {
  static bool attr = false;
  if (!attr) {
    if (!at_lds_attr((const void*)attn_tiled_bwd_q_kernel<DH, CAUSAL, DROP>, at_bwd_smem(DH)) ||
        !at_lds_attr((const void*)attn_tiled_bwd_kv_kernel<DH, CAUSAL, DROP>, at_bwd_smem(DH)))
      return VS_ERR_LAUNCH;
    attr = true;
  }
  const dim3 grid(a.R * a.H, (a.L + AP_QT - 1) / AP_QT);
  hipLaunchKernelGGL((attn_tiled_bwd_q_kernel<DH, CAUSAL, DROP>), grid, dim3(256), at_bwd_smem(DH), a.st, a.qkv, a.km,
                     a.dout, a.out, a.scratch, a.L, a.H, a.dr);
  hipLaunchKernelGGL((attn_tiled_bwd_kv_kernel<DH, CAUSAL, DROP>), grid, dim3(256), at_bwd_smem(DH), a.st, a.qkv, a.km,
                     a.dout, a.out, (const float*)a.scratch, a.L, a.H, a.dr);
  return VS_OK;
}

template <bool BWD, int DH, bool CAUSAL, bool DROP>
static int at_launch(const AtArgs& a) {
  return BWD ? at_bwd_launch<DH, CAUSAL, DROP>(a) : at_fwd_launch<DH, CAUSAL, DROP>(a);
}

template <bool BWD, int DH>
static int at_by_mode(const AtArgs& a, bool causal, bool drop) {
  if (causal) return drop ? at_launch<BWD, DH, true, true>(a) : at_launch<BWD, DH, true, false>(a);
  return drop ? at_launch<BWD, DH, false, true>(a) : at_launch<BWD, DH, false, false>(a);
}

template <bool BWD>
static int at_by_dh(const AtArgs& a, int dh, bool causal, bool drop) {
  switch (dh) {
    case 16: return at_by_mode<BWD, 16>(a, causal, drop);
    case 32: return at_by_mode<BWD, 32>(a, causal, drop);
    case 64: return at_by_mode<BWD, 64>(a, causal, drop);
    default: return at_by_mode<BWD, 128>(a, causal, drop);
  }
}

#define AT_CHECK_SHAPE()                                                                              \
  VS_CHECK_ARG(ap_dh_ok(dh), "head width must be 16, 32, 64 or 128");                                 \
  VS_CHECK_ARG((long long)R * H <= 0x7fffffffLL, "too many (sequence, head) pairs");                  \
  VS_CHECK_ARG(L <= AT_L_MAX, "sequence too long for the grid (and for 32-bit positions)");           \
  VS_CHECK_ARG((long long)H * dh * 3 <= 0x7fffffffLL, "3 * H * dh overflows a 32-bit index");         \
  VS_CHECK_ARG(snap || thr == 0, "a dropout threshold without the step's snapshot")

extern "C" int vs_attn_tiled_fwd(const float* qkv, const uint8_t* key_mask, float* out, int R, int L, int H, int dh,
                                 int causal, const int64_t* snap, uint32_t site, uint32_t thr, float scale,
                                 void* stream) {
  VS_CHECK_ARG(qkv && out && R > 0 && L > 0 && H > 0, "bad args");
  AT_CHECK_SHAPE();
  const AtArgs a{qkv, key_mask, nullptr, out, nullptr, R, L, H, DropArgs{snap, site, thr, scale}, (hipStream_t)stream};
  const int rc = at_by_dh<false>(a, dh, causal != 0, snap != nullptr);
  if (rc != VS_OK) return rc;
  VS_CHECK_LAUNCH();
  return VS_OK;
}

extern "C" size_t vs_attn_tiled_bwd_scratch_bytes(int R, int L, int H) {
  if (R <= 0 || L <= 0 || H <= 0) return 0;
  return (size_t)R * H * 3 * L * sizeof(float);
}

extern "C" int vs_attn_tiled_bwd(const float* qkv, const uint8_t* key_mask, const float* dout, float* dqkv,
                                 void* scratch, size_t scratch_bytes, int R, int L, int H, int dh, int causal,
                                 const int64_t* snap, uint32_t site, uint32_t thr, float scale, void* stream) {
  VS_CHECK_ARG(qkv && dout && dqkv && scratch && R > 0 && L > 0 && H > 0, "bad args");
  AT_CHECK_SHAPE();
  VS_CHECK_ARG(scratch_bytes >= vs_attn_tiled_bwd_scratch_bytes(R, L, H), "scratch too small");
  VS_CHECK_ARG(((uintptr_t)scratch & 3) == 0, "scratch must be 4-byte aligned");
  const AtArgs a{qkv, key_mask, dout, dqkv, (float*)scratch, R, L, H, DropArgs{snap, site, thr, scale},
                 (hipStream_t)stream};
  const int rc = at_by_dh<true>(a, dh, causal != 0, snap != nullptr);
  if (rc != VS_OK) return rc;
  VS_CHECK_LAUNCH();
  return VS_OK;
}

// 1 where the LDS-resident kernel of this rule and direction holds (L, dh) -- by the formulas its launcher checks.
extern "C" int vs_attn_resident_fits(int causal, int L, int dh, int backward) {
  if (L <= 0 || dh <= 0) return 0;
  if (causal)
    return backward ? (ac_bwd_q_smem(L, dh) <= AC_LDS_MAX && ac_bwd_kv_smem(L, dh) <= AC_LDS_MAX)
                    : ac_fwd_smem(L, dh) <= AC_LDS_MAX;
  if (!ap_dh_ok(dh)) return 0;
  return (backward ? ap_bwd_smem(L, dh) : ap_fwd_smem(L, dh)) <= AP_LDS_MAX;
}
