// RoBERTa encoder kernels (fp32): bidirectional padding-masked self-attention on the exact-fp32 matrix
// instruction (forward and backward), the RoBERTa embedding rule, erf GELU and tanh.
// Semantics are those of huggingface transformers 3.3.1 (modeling_roberta / modeling_bert), the release
// the reference pins.
#include <math.h>

#include "attn_shared.h"
#include "common.h"

// ----------------------------------------------------------------------------
// Self-attention over a fused qkv buffer [R, L, 3D]:
//   s_ij = q_i . k_j / sqrt(dh) + (1 - mask[r, j]) * -1e4   (get_extended_attention_mask),
//   p = softmax over all L keys, out = p v with the heads merged.  Not causal; queries at padded positions are
//   computed like any other.  Lp = L rounded up to the 16-wide tile: columns j >= L take no part (weight exactly 0,
//   never in the row maximum).
// One block per (sequence, head, 64 queries).  The head's K and V are staged once in LDS (pitch dh + 4: the 16 x 4
// operand reads of v_mfma_f32_16x16x4_f32 then touch 64 different banks); each of the four waves owns 16 queries:
// its Q fragments live in registers, its score tile [16][Lp] in a private LDS strip, never in memory.
// Operand maps of the instruction: A[lane & 15][lane >> 4], B[lane >> 4][lane & 15], D[(lane >> 4) * 4 + reg][lane & 15].
// ----------------------------------------------------------------------------
// (attn_shared.h: AP_QT, AP_LDS_MAX, mfma4, ap_stage, ap_any_key_valid -- the masking rule --, ap_mask4 -- the dropout
// draw --, and the LDS formulas ap_fwd_smem / ap_bwd_smem)

template <int DH, bool DROP>
__global__ __launch_bounds__(256) void attn_pad_fwd_kernel(const float* __restrict__ qkv,
                                                           const uint8_t* __restrict__ kmask,
                                                           float* __restrict__ out, int L, int Lp, int H,
                                                           DropArgs dr) {
  extern __shared__ float sm[];
  constexpr int LD = DH + 4, KS = DH / 4, CT = DH / 16;
  const int D = H * DH, LS = Lp + 4;
  const int r = blockIdx.x / H, h = blockIdx.x % H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  float* Ks = sm;
  float* Vs = Ks + Lp * LD;
  float* Sw = Vs + Lp * LD + wave * 16 * LS;  // this wave's scores [16][LS]
  const float* base = qkv + (long long)r * L * 3 * D + h * DH;
  ap_stage<DH>(Ks, base + D, 3LL * D, L, Lp);
  ap_stage<DH>(Vs, base + 2 * D, 3LL * D, L, Lp);
  const int i0 = blockIdx.y * AP_QT + wave * 16;
  const bool active = i0 < L;  // wave-uniform
  float qf[KS];
  {
    const int i = i0 + lr;
#pragma unroll
    for (int k = 0; k < KS; ++k) qf[k] = i < L ? base[(long long)i * 3 * D + k * 4 + lq] : 0.f;
  }
  const bool masked = ap_any_key_valid(kmask, r, L);  // its block barrier also ends the staging of K and V
  const float scale = 1.0f / sqrtf((float)DH);
  if (active) {
    for (int jt = 0; jt < Lp / 16; ++jt) {
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};  // even / odd k steps: two independent chains
      const float* kp = Ks + (jt * 16 + lr) * LD + lq;
#pragma unroll
      for (int k = 0; k < KS; k += 2) {
        a0 = mfma4(qf[k], kp[k * 4], a0);
        a1 = mfma4(qf[k + 1], kp[k * 4 + 4], a1);
      }
      const int j = jt * 16 + lr;
      const bool off = masked && j < L && !kmask[(long long)r * L + j];
#pragma unroll
      for (int g = 0; g < 4; ++g) Sw[(lq * 4 + g) * LS + j] = off ? -INFINITY : (a0[g] + a1[g]) * scale;
    }
  }
  __syncthreads();
  float inv = 0.f;
  if (active) {  // softmax: four lanes per row
    float* row = Sw + (lane >> 2) * LS;
    const int c0 = lane & 3;
    float mx = -INFINITY;
    for (int c = c0; c < L; c += 4) mx = fmaxf(mx, row[c]);
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    float sum = 0.f;
    for (int c = c0; c < L; c += 4) {
      const float e = expf(row[c] - mx);
      row[c] = e;
      sum += e;
    }
    for (int c = L + c0; c < Lp; c += 4) row[c] = 0.f;
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    inv = 1.0f / sum;
    if (DROP) {  // e_ij *= m_ij; the row sum above is the undropped one
      __builtin_amdgcn_wave_barrier();  // the row's other three lanes wrote what this lane reads
      const int i = i0 + (lane >> 2);
      if (i < L) {
        const uint64_t seed = (uint64_t)dr.snap[0], step = (uint64_t)dr.snap[1];
        const uint64_t rowblk = ((uint64_t)blockIdx.x * L + i) * (uint64_t)((L + 3) >> 2);
        for (int b = c0; b * 4 < L; b += 4) {  // columns L .. 4b + 3 of the last block hold 0 and stay 0
          const float4 m = ap_mask4(dr, seed, step, rowblk, b);
          float4 e = *(float4*)(row + b * 4);
          e.x *= m.x; e.y *= m.y; e.z *= m.z; e.w *= m.w;
          *(float4*)(row + b * 4) = e;
        }
      }
    }
  }
  __syncthreads();
  if (active) {
    f32x4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < Lp / 4; ++k) {
      const float a = Sw[lr * LS + k * 4 + lq];
      const float* vp = Vs + (k * 4 + lq) * LD + lr;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[ct] = mfma4(a, vp[ct * 16], acc[ct]);
    }
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

static bool ap_lds_attr(const void* kernel) {
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, AP_LDS_MAX);
  if (e == hipSuccess) return true;
  (void)hipGetLastError();
  vs_set_error("attention kernel refused %d bytes of dynamic LDS: %s", AP_LDS_MAX, hipGetErrorString(e));
  return false;
}

template <int DH, bool DROP>
static int ap_fwd_launch(const float* qkv, const uint8_t* km, float* out, int R, int L, int H, size_t smem,
                         DropArgs dr, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    if (!ap_lds_attr((const void*)attn_pad_fwd_kernel<DH, DROP>)) return VS_ERR_LAUNCH;
    attr = true;
  }
  hipLaunchKernelGGL((attn_pad_fwd_kernel<DH, DROP>), dim3(R * H, (L + AP_QT - 1) / AP_QT), dim3(256), smem, st, qkv,
                     km, out, L, ap_lp(L), H, dr);
  return VS_OK;
}

template <bool DROP>
static int ap_fwd(const float* qkv, const uint8_t* key_mask, float* out, int R, int L, int H, int dh, DropArgs dr,
                  void* stream) {
  VS_CHECK_ARG(qkv && out && R > 0 && L > 0 && H > 0, "bad args");
  VS_CHECK_ARG(ap_dh_ok(dh), "head width must be 16, 32, 64 or 128");
  VS_CHECK_ARG((long long)R * H <= 0x7fffffffLL, "too many (sequence, head) pairs");
  const size_t smem = ap_fwd_smem(L, dh);
  VS_CHECK_ARG(smem <= AP_LDS_MAX, "sequence too long for the LDS-resident attention (L*dh)");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  switch (dh) {
    case 16: rc = ap_fwd_launch<16, DROP>(qkv, key_mask, out, R, L, H, smem, dr, st); break;
    case 32: rc = ap_fwd_launch<32, DROP>(qkv, key_mask, out, R, L, H, smem, dr, st); break;
    case 64: rc = ap_fwd_launch<64, DROP>(qkv, key_mask, out, R, L, H, smem, dr, st); break;
    default: rc = ap_fwd_launch<128, DROP>(qkv, key_mask, out, R, L, H, smem, dr, st); break;
  }
  if (rc != VS_OK) return rc;
  VS_CHECK_LAUNCH();
  return VS_OK;
}

extern "C" int vs_attn_pad_fwd(const float* qkv, const uint8_t* key_mask, float* out, int R, int L, int H, int dh,
                               void* stream) {
  return ap_fwd<false>(qkv, key_mask, out, R, L, H, dh, DropArgs{}, stream);
}

extern "C" int vs_attn_pad_drop_fwd(const float* qkv, const uint8_t* key_mask, float* out, int R, int L, int H,
                                    int dh, const int64_t* snap, uint32_t site, uint32_t thr, float scale,
                                    void* stream) {
  VS_CHECK_ARG(snap, "bad args");
  return ap_fwd<true>(qkv, key_mask, out, R, L, H, dh, DropArgs{snap, site, thr, scale}, stream);
}

// ----------------------------------------------------------------------------
// Backward in two launches, p recomputed from q, k and the mask (the forward stores nothing):
// Launch A (64 queries per block, 16 per wave): s, p as the forward; dP = dO V^T beside it on the matrix unit;
//   D_i = sum_j p_ij dP_ij (= rowsum(dO * O)); dS = p * (dP - D_i); dQ = scale * dS K.  The p and dS rows go to the
//   scratch [R*H][2][L][Lp] (columns j >= L are zero).
// Launch B (64 keys per block, 16 per wave): Q and dO of the head in LDS, the wave's columns of p / dS are the A
//   operand read straight from the scratch: dV = P^T dO, dK = scale * dS^T Q.
// Every output element has one owner and a fixed summation order (k-ordered fma chains of the instruction): no
// atomics, two runs agree bit for bit.
// DROP (out = (p o m) v, the mask regenerated from the step's snapshot as in the forward): dP = m o (dO V^T), D and dS
// as above from the undropped p, and the scratch's p rows hold p o m -- launch A writes them from the mask pass, where
// a lane has both -- so that launch B (dV = (p o m)^T dO) is the plain one.
// ----------------------------------------------------------------------------
template <int DH, bool DROP>
__global__ __launch_bounds__(256) void attn_pad_bwd_q_kernel(const float* __restrict__ qkv,
                                                             const uint8_t* __restrict__ kmask,
                                                             const float* __restrict__ dout,
                                                             float* __restrict__ dqkv, float* __restrict__ scratch,
                                                             int L, int Lp, int H, DropArgs dr) {
  extern __shared__ float sm[];
  constexpr int LD = DH + 4, KS = DH / 4, CT = DH / 16;
  const int D = H * DH, LS = Lp + 4;
  const int r = blockIdx.x / H, h = blockIdx.x % H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  float* Ks = sm;
  float* Vs = Ks + Lp * LD;
  float* Pw = Vs + Lp * LD + wave * 32 * LS;  // p  [16][LS]
  float* Dw = Pw + 16 * LS;                   // dP, then dS
  const float* base = qkv + (long long)r * L * 3 * D + h * DH;
  const float* dob = dout + (long long)r * L * D + h * DH;
  float* Pg = scratch + (long long)blockIdx.x * 2 * L * Lp;
  float* Sg = Pg + (long long)L * Lp;
  ap_stage<DH>(Ks, base + D, 3LL * D, L, Lp);
  ap_stage<DH>(Vs, base + 2 * D, 3LL * D, L, Lp);
  const int i0 = blockIdx.y * AP_QT + wave * 16;
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
  const bool masked = ap_any_key_valid(kmask, r, L);  // its block barrier also ends the staging of K and V
  const float scale = 1.0f / sqrtf((float)DH);
  if (active) {
    for (int jt = 0; jt < Lp / 16; ++jt) {
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f}, b0 = {0.f, 0.f, 0.f, 0.f};
      const float* kp = Ks + (jt * 16 + lr) * LD + lq;
      const float* vp = Vs + (jt * 16 + lr) * LD + lq;
#pragma unroll
      for (int k = 0; k < KS; k += 2) {  // the score in the forward's own order
        a0 = mfma4(qf[k], kp[k * 4], a0);
        a1 = mfma4(qf[k + 1], kp[k * 4 + 4], a1);
        b0 = mfma4(of[k], vp[k * 4], b0);
        b0 = mfma4(of[k + 1], vp[k * 4 + 4], b0);
      }
      const int j = jt * 16 + lr;
      const bool off = masked && j < L && !kmask[(long long)r * L + j];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        Pw[(lq * 4 + g) * LS + j] = off ? -INFINITY : (a0[g] + a1[g]) * scale;
        Dw[(lq * 4 + g) * LS + j] = b0[g];
      }
    }
  }
  __syncthreads();
  if (active) {
    float* row = Pw + (lane >> 2) * LS;
    float* drow = Dw + (lane >> 2) * LS;
    const int c0 = lane & 3;
    float mx = -INFINITY;
    for (int c = c0; c < L; c += 4) mx = fmaxf(mx, row[c]);
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    float sum = 0.f;
    for (int c = c0; c < L; c += 4) {
      const float e = expf(row[c] - mx);
      row[c] = e;
      sum += e;
    }
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    const float inv = 1.0f / sum;
    float dsum = 0.f;
    if (DROP) {
      __builtin_amdgcn_wave_barrier();  // the row's other three lanes wrote what this lane reads
      const int i = i0 + (lane >> 2);
      const bool live = i < L;  // a row past L owns no scratch row and no output; its strip is never read for one
      const uint64_t seed = (uint64_t)dr.snap[0], step = (uint64_t)dr.snap[1];
      const uint64_t rowblk = ((uint64_t)blockIdx.x * L + (live ? i : 0)) * (uint64_t)((L + 3) >> 2);
      float4* pg4 = (float4*)(Pg + (long long)(live ? i : 0) * Lp);
      if (live)
        for (int b = c0; b < Lp / 4; b += 4) {  // blocks, not strided columns; the blocks past L are zero
          const int j = b * 4;
          float4 p = make_float4(0.f, 0.f, 0.f, 0.f), g = p, pm = p;
          if (j < L) {
            const float4 m = ap_mask4(dr, seed, step, rowblk, b);
            const float4 e = *(const float4*)(row + j), d = *(const float4*)(drow + j);
            p.x = e.x * inv;
            g.x = m.x * d.x;
            pm.x = p.x * m.x;
            if (j + 1 < L) { p.y = e.y * inv; g.y = m.y * d.y; pm.y = p.y * m.y; }
            if (j + 2 < L) { p.z = e.z * inv; g.z = m.z * d.z; pm.z = p.z * m.z; }
            if (j + 3 < L) { p.w = e.w * inv; g.w = m.w * d.w; pm.w = p.w * m.w; }
            dsum += (p.x * g.x + p.y * g.y) + (p.z * g.z + p.w * g.w);
          }
          *(float4*)(row + j) = p;
          *(float4*)(drow + j) = g;
          pg4[b] = pm;
        }
      dsum += __shfl_xor(dsum, 1, 64);
      dsum += __shfl_xor(dsum, 2, 64);
      if (live)
        for (int b = c0; b * 4 < L; b += 4) {  // the same lane's own blocks: dS = p (dP - D); p = 0 past L
          const float4 p = *(const float4*)(row + b * 4);
          float4 g = *(const float4*)(drow + b * 4);
          g.x = p.x * (g.x - dsum); g.y = p.y * (g.y - dsum); g.z = p.z * (g.z - dsum); g.w = p.w * (g.w - dsum);
          *(float4*)(drow + b * 4) = g;
        }
    } else {
      for (int c = c0; c < L; c += 4) {
        const float p = row[c] * inv;
        row[c] = p;
        dsum += p * drow[c];
      }
      dsum += __shfl_xor(dsum, 1, 64);
      dsum += __shfl_xor(dsum, 2, 64);
      for (int c = c0; c < L; c += 4) drow[c] = row[c] * (drow[c] - dsum);
      for (int c = L + c0; c < Lp; c += 4) {
        row[c] = 0.f;
        drow[c] = 0.f;
      }
    }
  }
  __syncthreads();
  if (active) {
    for (int rw = 0; rw < 16; ++rw) {
      const int i = i0 + rw;
      if (i >= L) break;
      for (int c = lane; c < Lp; c += 64) {
        if (!DROP) Pg[(long long)i * Lp + c] = Pw[rw * LS + c];  // DROP: p o m went out from the mask pass
        Sg[(long long)i * Lp + c] = Dw[rw * LS + c];
      }
    }
    f32x4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < Lp / 4; ++k) {
      const float a = Dw[lr * LS + k * 4 + lq];
      const float* kp = Ks + (k * 4 + lq) * LD + lr;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[ct] = mfma4(a, kp[ct * 16], acc[ct]);
    }
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

template <int DH>
__global__ __launch_bounds__(256) void attn_pad_bwd_kv_kernel(const float* __restrict__ qkv,
                                                              const float* __restrict__ dout,
                                                              float* __restrict__ dqkv,
                                                              const float* __restrict__ scratch, int L, int Lp,
                                                              int H) {
  extern __shared__ float sm[];
  constexpr int LD = DH + 4, CT = DH / 16;
  const int D = H * DH;
  const int r = blockIdx.x / H, h = blockIdx.x % H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  float* Qs = sm;
  float* Os = Qs + Lp * LD;
  const float* base = qkv + (long long)r * L * 3 * D + h * DH;
  const float* dob = dout + (long long)r * L * D + h * DH;
  const float* Pg = scratch + (long long)blockIdx.x * 2 * L * Lp;
  const float* Sg = Pg + (long long)L * Lp;
  ap_stage<DH>(Qs, base, 3LL * D, L, Lp);
  ap_stage<DH>(Os, dob, (long long)D, L, Lp);
  __syncthreads();
  const int j0 = blockIdx.y * AP_QT + wave * 16;
  if (j0 >= L) return;  // (no barrier below)
  const float scale = 1.0f / sqrtf((float)DH);
  f32x4 av[CT], ak[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) av[ct] = ak[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < Lp / 4; ++k) {
    const int i = k * 4 + lq;
    float ap = 0.f, as = 0.f;
    if (i < L) {  // column j0 + lr < Lp: inside the scratch row
      ap = Pg[(long long)i * Lp + j0 + lr];
      as = Sg[(long long)i * Lp + j0 + lr];
    }
    const float* op = Os + i * LD + lr;
    const float* qp = Qs + i * LD + lr;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      av[ct] = mfma4(ap, op[ct * 16], av[ct]);
      ak[ct] = mfma4(as, qp[ct * 16], ak[ct]);
    }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int j = j0 + lq * 4 + g;
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

extern "C" size_t vs_attn_pad_bwd_scratch_bytes(int R, int L, int H) {
  if (R <= 0 || L <= 0 || H <= 0) return 0;
  return (size_t)R * H * 2 * L * ap_lp(L) * sizeof(float);
}

template <int DH, bool DROP>
static int ap_bwd_launch(const float* qkv, const uint8_t* km, const float* dout, float* dqkv, float* scratch,
                          int R, int L, int H, DropArgs dr, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    if (!ap_lds_attr((const void*)attn_pad_bwd_q_kernel<DH, DROP>) ||
        !ap_lds_attr((const void*)attn_pad_bwd_kv_kernel<DH>))
      return VS_ERR_LAUNCH;
    attr = true;
  }
  const int Lp = ap_lp(L);
  const dim3 grid(R * H, (L + AP_QT - 1) / AP_QT);
  hipLaunchKernelGGL((attn_pad_bwd_q_kernel<DH, DROP>), grid, dim3(256), ap_bwd_smem(L, DH), st, qkv, km, dout, dqkv,
                     scratch, L, Lp, H, dr);
  hipLaunchKernelGGL(attn_pad_bwd_kv_kernel<DH>, grid, dim3(256), (size_t)2 * Lp * (DH + 4) * sizeof(float), st,
                     qkv, dout, dqkv, (const float*)scratch, L, Lp, H);
  return VS_OK;
}

template <bool DROP>
static int ap_bwd(const float* qkv, const uint8_t* key_mask, const float* dout, float* dqkv, void* scratch,
                  size_t scratch_bytes, int R, int L, int H, int dh, DropArgs dr, void* stream) {
  VS_CHECK_ARG(qkv && dout && dqkv && scratch && R > 0 && L > 0 && H > 0, "bad args");
  VS_CHECK_ARG(ap_dh_ok(dh), "head width must be 16, 32, 64 or 128");
  VS_CHECK_ARG((long long)R * H <= 0x7fffffffLL, "too many (sequence, head) pairs");
  VS_CHECK_ARG(ap_bwd_smem(L, dh) <= AP_LDS_MAX, "sequence too long for the LDS-resident attention backward (L*dh)");
  VS_CHECK_ARG(scratch_bytes >= vs_attn_pad_bwd_scratch_bytes(R, L, H), "scratch too small");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  switch (dh) {
    case 16: rc = ap_bwd_launch<16, DROP>(qkv, key_mask, dout, dqkv, (float*)scratch, R, L, H, dr, st); break;
    case 32: rc = ap_bwd_launch<32, DROP>(qkv, key_mask, dout, dqkv, (float*)scratch, R, L, H, dr, st); break;
    case 64: rc = ap_bwd_launch<64, DROP>(qkv, key_mask, dout, dqkv, (float*)scratch, R, L, H, dr, st); break;
    default: rc = ap_bwd_launch<128, DROP>(qkv, key_mask, dout, dqkv, (float*)scratch, R, L, H, dr, st); break;
  }
  if (rc != VS_OK) return rc;
  VS_CHECK_LAUNCH();
  return VS_OK;
}

extern "C" int vs_attn_pad_bwd(const float* qkv, const uint8_t* key_mask, const float* dout, float* dqkv,
                               void* scratch, size_t scratch_bytes, int R, int L, int H, int dh, void* stream) {
  return ap_bwd<false>(qkv, key_mask, dout, dqkv, scratch, scratch_bytes, R, L, H, dh, DropArgs{}, stream);
}

extern "C" int vs_attn_pad_drop_bwd(const float* qkv, const uint8_t* key_mask, const float* dout, float* dqkv,
                                    void* scratch, size_t scratch_bytes, int R, int L, int H, int dh,
                                    const int64_t* snap, uint32_t site, uint32_t thr, float scale, void* stream) {
  VS_CHECK_ARG(snap, "bad args");
  VS_CHECK_ARG(((uintptr_t)scratch & 15) == 0, "scratch must be 16-byte aligned");
  return ap_bwd<true>(qkv, key_mask, dout, dqkv, scratch, scratch_bytes, R, L, H, dh, DropArgs{snap, site, thr, scale},
                      stream);
}

// ----------------------------------------------------------------------------
// RobertaEmbeddings before its LayerNorm: position ids from the token ids (create_position_ids_from_input_ids):
//   pos_id[l] = cumsum(tokens != pad)[l] * (tokens[l] != pad) + pad;  out = word[tok] + pos[pos_id] + type0.
// One block per token; the count of non-padding tokens up to l is an integer block reduction (exact).
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void roberta_embed_kernel(const int64_t* __restrict__ tok,
                                                            const float* __restrict__ word,
                                                            const float* __restrict__ pos,
                                                            const float* __restrict__ type0,
                                                            float* __restrict__ out, int64_t* __restrict__ pos_ids,
                                                            int L, int D, long long pad, int n_pos) {
  __shared__ int part[4];
  const int row = blockIdx.x;
  const int r = row / L, l = row - r * L;
  const int64_t* t = tok + (long long)r * L;
  int cnt = 0;
  for (int i = threadIdx.x; i <= l; i += 256) cnt += t[i] != pad ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  cnt = part[0] + part[1] + part[2] + part[3];
  long long tk = t[l];
  long long pid = (tk != pad ? (long long)cnt : 0LL) + pad;
  if (pid >= n_pos) pid = n_pos - 1;  // never with the host's L + pad + 1 <= n_pos; keeps the read inside the table
  if (tk < 0) tk = 0;
  if (threadIdx.x == 0) pos_ids[row] = pid;
  const float4* a = (const float4*)(word + tk * D);
  const float4* p = (const float4*)(pos + pid * D);
  const float4* ty = (const float4*)type0;
  float4* o = (float4*)(out + (long long)row * D);
  for (int i = threadIdx.x; i < D / 4; i += 256) {
    const float4 u = a[i], v = p[i], w = ty[i];
    o[i] = make_float4(u.x + v.x + w.x, u.y + v.y + w.y, u.z + v.z + w.z, u.w + v.w + w.w);
  }
}

extern "C" int vs_roberta_embed(const int64_t* tokens, const float* word, const float* pos, const float* type0,
                                float* out, int64_t* pos_ids_out, int R, int L, int D, int pad, int n_pos,
                                void* stream) {
  VS_CHECK_ARG(tokens && word && pos && type0 && out && pos_ids_out && R > 0 && L > 0 && D > 0 && D % 4 == 0 &&
                   pad >= 0, "bad args");
  VS_CHECK_ARG((long long)L + pad + 1 <= n_pos, "sequence longer than the position table (L + pad + 1 > n_pos)");
  VS_CHECK_ARG((long long)R * L <= 0x7fffffffLL, "too many tokens");
  hipLaunchKernelGGL(roberta_embed_kernel, dim3(R * L), dim3(256), 0, (hipStream_t)stream, tokens, word, pos, type0,
                     out, pos_ids_out, L, D, (long long)pad, n_pos);
  VS_CHECK_LAUNCH();
  return VS_OK;
}

// ----------------------------------------------------------------------------
// gelu(x) = x * 0.5 * (1 + erf(x / sqrt(2)))  (roberta's hidden_act "gelu"), tanh (pooler, classification head)
// ----------------------------------------------------------------------------
__global__ void gelu_erf_fwd_kernel(const float* x, float* y, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float v = x[i];
    y[i] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
  }
}
__global__ void gelu_erf_bwd_kernel(const float* dy, const float* x, float* dx, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float v = x[i];
    const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752f));
    const float pdf = 0.39894228040143268f * expf(-0.5f * v * v);
    dx[i] = dy[i] * (cdf + v * pdf);
  }
}
__global__ void tanh_fwd_kernel(const float* x, float* y, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    y[i] = tanhf(x[i]);
}
__global__ void tanh_bwd_kernel(const float* dy, const float* y, float* dx, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float t = y[i];
    dx[i] = dy[i] * (1.0f - t * t);
  }
}
static inline unsigned rb_blocks(long long n) {
  long long g = (n + 255) / 256;
  if (g > 4096) g = 4096;
  return (unsigned)(g < 1 ? 1 : g);
}
extern "C" int vs_gelu_erf_fwd(const float* x, float* y, int64_t n, void* stream) {
  VS_CHECK_ARG(x && y && n > 0, "bad args");
  hipLaunchKernelGGL(gelu_erf_fwd_kernel, dim3(rb_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)n);
  VS_CHECK_LAUNCH();
  return VS_OK;
}
extern "C" int vs_gelu_erf_bwd(const float* dy, const float* x_pre, float* dx, int64_t n, void* stream) {
  VS_CHECK_ARG(dy && x_pre && dx && n > 0, "bad args");
  hipLaunchKernelGGL(gelu_erf_bwd_kernel, dim3(rb_blocks(n)), dim3(256), 0, (hipStream_t)stream, dy, x_pre, dx,
                     (long long)n);
  VS_CHECK_LAUNCH();
  return VS_OK;
}
extern "C" int vs_tanh_fwd(const float* x, float* y, int64_t n, void* stream) {
  VS_CHECK_ARG(x && y && n > 0, "bad args");
  hipLaunchKernelGGL(tanh_fwd_kernel, dim3(rb_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)n);
  VS_CHECK_LAUNCH();
  return VS_OK;
}
extern "C" int vs_tanh_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream) {
  VS_CHECK_ARG(dy && y && dx && n > 0, "bad args");
  hipLaunchKernelGGL(tanh_bwd_kernel, dim3(rb_blocks(n)), dim3(256), 0, (hipStream_t)stream, dy, y, dx, (long long)n);
  VS_CHECK_LAUNCH();
  return VS_OK;
}
