// Encoder (cross) attention of the fairseq decoder (fp32): L queries of a row attend over the S keys of that row's
// source, queries and keys from different tensors.  Forward, backward and a one-query cached decode step, all on the
// exact-fp32 matrix instruction or plain fp32 FMAs; the layout and the masking rule are those of roberta_ops.hip.
//   q [R*L, D] (D = H * dh), kv [R*S, 2D] (k | v, one GEMM on the concatenated [2D, D] weight), key_mask u8 [R, S]
//   (1 = valid) or NULL:  s_ij = q_i . k_j / sqrt(dh) (fairseq scales q after its projection, bias included),
//   p = softmax over the S keys, out = p v with the heads merged.  Not causal, no dropout on the probabilities.
// Masked keys weigh exactly 0; a row whose mask is all zero runs unmasked (ap_any_key_valid; fairseq gives NaN there).
// Sp = S rounded up to the 16-wide tile: columns j >= S take no part.
#include <math.h>

#include "attn_shared.h"
#include "common.h"

// ----------------------------------------------------------------------------
// Forward: one block per (row, head, 64 queries); the head's K and V staged once in LDS at pitch dh + 4; each of the four
// waves owns 16 queries: Q fragments in registers, the score tile [16][Sp] in a private LDS strip, never in memory.
// LDS: ap_fwd_smem(S, dh).
// ----------------------------------------------------------------------------
template <int DH>
__global__ __launch_bounds__(256) void attn_cross_fwd_kernel(const float* __restrict__ q,
                                                             const float* __restrict__ kv,
                                                             const uint8_t* __restrict__ kmask,
                                                             float* __restrict__ out, int L, int S, int Sp, int H) {
  extern __shared__ float sm[];
  constexpr int LD = DH + 4, KS = DH / 4, CT = DH / 16;
  const int D = H * DH, LS = Sp + 4;
  const int r = blockIdx.x / H, h = blockIdx.x % H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  float* Ks = sm;
  float* Vs = Ks + Sp * LD;
  float* Sw = Vs + Sp * LD + wave * 16 * LS;  // this wave's scores [16][LS]
  const float* qb = q + (long long)r * L * D + h * DH;
  const float* kb = kv + (long long)r * S * 2 * D + h * DH;
  ap_stage<DH>(Ks, kb, 2LL * D, S, Sp);
  ap_stage<DH>(Vs, kb + D, 2LL * D, S, Sp);
  const int i0 = blockIdx.y * AP_QT + wave * 16;
  const bool active = i0 < L;  // wave-uniform
  float qf[KS];
  {
    const int i = i0 + lr;
#pragma unroll
    for (int k = 0; k < KS; ++k) qf[k] = i < L ? qb[(long long)i * D + k * 4 + lq] : 0.f;
  }
  const bool masked = ap_any_key_valid(kmask, r, S);  // its block barrier also ends the staging of K and V
  const float scale = 1.0f / sqrtf((float)DH);
  if (active) {
    for (int jt = 0; jt < Sp / 16; ++jt) {
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};  // even / odd k steps: two independent chains
      const float* kp = Ks + (jt * 16 + lr) * LD + lq;
#pragma unroll
      for (int k = 0; k < KS; k += 2) {
        a0 = mfma4(qf[k], kp[k * 4], a0);
        a1 = mfma4(qf[k + 1], kp[k * 4 + 4], a1);
      }
      const int j = jt * 16 + lr;
      const bool off = masked && j < S && !kmask[(long long)r * S + j];
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
    for (int c = c0; c < S; c += 4) mx = fmaxf(mx, row[c]);
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    float sum = 0.f;
    for (int c = c0; c < S; c += 4) {
      const float e = expf(row[c] - mx);
      row[c] = e;
      sum += e;
    }
    for (int c = S + c0; c < Sp; c += 4) row[c] = 0.f;
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    inv = 1.0f / sum;
  }
  __syncthreads();
  if (active) {
    f32x4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < Sp / 4; ++k) {
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

static bool ax_lds_attr(const void* kernel) {
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, AP_LDS_MAX);
  if (e == hipSuccess) return true;
  (void)hipGetLastError();
  vs_set_error("cross attention kernel refused %d bytes of dynamic LDS: %s", AP_LDS_MAX, hipGetErrorString(e));
  return false;
}

// the shape checks every entry point of the family makes; nothing is written when one fails
static int ax_check_shape(const char* fn, int R, int L, int S, int H, int dh, bool backward) {
  if (!(R > 0 && L > 0 && S > 0 && H > 0)) {
    vs_set_error("%s: bad args", fn);
    return VS_ERR_BAD_ARG;
  }
  if (!ap_dh_ok(dh)) {
    vs_set_error("%s: head width must be 16, 32, 64 or 128", fn);
    return VS_ERR_BAD_ARG;
  }
  if ((long long)R * H > 0x7fffffffLL || (L + AP_QT - 1) / AP_QT > 65535) {
    vs_set_error("%s: too many (row, head) pairs or query tiles", fn);
    return VS_ERR_BAD_ARG;
  }
  const size_t need = backward ? ap_bwd_smem(S, dh) : ap_fwd_smem(S, dh);
  if (need > AP_LDS_MAX) {
    vs_set_error("%s: source too long for the LDS-resident cross attention: S = %d at dh = %d needs %zu bytes of LDS, "
                 "the limit is %d", fn, S, dh, need, AP_LDS_MAX);
    return VS_ERR_BAD_ARG;
  }
  return VS_OK;
}

template <int DH>
static int ax_fwd_launch(const float* q, const float* kv, const uint8_t* km, float* out, int R, int L, int S, int H,
                         hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    if (!ax_lds_attr((const void*)attn_cross_fwd_kernel<DH>)) return VS_ERR_LAUNCH;
    attr = true;
  }
  hipLaunchKernelGGL(attn_cross_fwd_kernel<DH>, dim3(R * H, (L + AP_QT - 1) / AP_QT), dim3(256), ap_fwd_smem(S, DH),
                     st, q, kv, km, out, L, S, ap_lp(S), H);
  return VS_OK;
}

extern "C" int vs_attn_cross_fwd(const float* q, const float* kv, const uint8_t* key_mask, float* out, int R, int L,
                                 int S, int H, int dh, void* stream) {
  VS_CHECK_ARG(q && kv && out, "bad args");
  int rc = ax_check_shape(__func__, R, L, S, H, dh, false);
  if (rc != VS_OK) return rc;
  VS_CHECK_ARG((((uintptr_t)kv) & 15) == 0, "kv must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  switch (dh) {
    case 16: rc = ax_fwd_launch<16>(q, kv, key_mask, out, R, L, S, H, st); break;
    case 32: rc = ax_fwd_launch<32>(q, kv, key_mask, out, R, L, S, H, st); break;
    case 64: rc = ax_fwd_launch<64>(q, kv, key_mask, out, R, L, S, H, st); break;
    default: rc = ax_fwd_launch<128>(q, kv, key_mask, out, R, L, S, H, st); break;
  }
  if (rc != VS_OK) return rc;
  VS_CHECK_LAUNCH();
  return VS_OK;
}

// ----------------------------------------------------------------------------
// Backward in two launches, p recomputed from q, k and the mask (the forward stores nothing):
// Launch A (64 queries per block, 16 per wave): s, p as the forward; dP = dO V^T beside it on the matrix unit;
//   D_i = sum_j p_ij dP_ij; dS = p * (dP - D_i); dQ = scale * dS K.  The p and dS rows go to the scratch
//   [R*H][2][L][Sp] (columns j >= S are zero).  LDS: ap_bwd_smem(S, dh).
// Launch B (64 keys per block, 16 per wave): Q and dO of the head pass through LDS 64 queries at a time, in ascending
//   order; the wave's columns of p / dS are the A operand read straight from the scratch: dV = P^T dO,
//   dK = scale * dS^T Q.  LDS: ax_bwd_kv_smem(dh), whatever L and S.
// Every element of dq, dkv and of the scratch that is read has one owner that writes it first, and a fixed summation
// order: no atomics, two runs agree bit for bit.
// ----------------------------------------------------------------------------
template <int DH>
__global__ __launch_bounds__(256) void attn_cross_bwd_q_kernel(const float* __restrict__ q,
                                                               const float* __restrict__ kv,
                                                               const uint8_t* __restrict__ kmask,
                                                               const float* __restrict__ dout,
                                                               float* __restrict__ dq, float* __restrict__ scratch,
                                                               int L, int S, int Sp, int H) {
  extern __shared__ float sm[];
  constexpr int LD = DH + 4, KS = DH / 4, CT = DH / 16;
  const int D = H * DH, LS = Sp + 4;
  const int r = blockIdx.x / H, h = blockIdx.x % H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  float* Ks = sm;
  float* Vs = Ks + Sp * LD;
  float* Pw = Vs + Sp * LD + wave * 32 * LS;  // p  [16][LS]
  float* Dw = Pw + 16 * LS;                   // dP, then dS
  const float* qb = q + (long long)r * L * D + h * DH;
  const float* dob = dout + (long long)r * L * D + h * DH;
  const float* kb = kv + (long long)r * S * 2 * D + h * DH;
  float* Pg = scratch + (long long)blockIdx.x * 2 * L * Sp;
  float* Sg = Pg + (long long)L * Sp;
  ap_stage<DH>(Ks, kb, 2LL * D, S, Sp);
  ap_stage<DH>(Vs, kb + D, 2LL * D, S, Sp);
  const int i0 = blockIdx.y * AP_QT + wave * 16;
  const bool active = i0 < L;
  float qf[KS], of[KS];
  {
    const int i = i0 + lr;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      qf[k] = i < L ? qb[(long long)i * D + k * 4 + lq] : 0.f;
      of[k] = i < L ? dob[(long long)i * D + k * 4 + lq] : 0.f;
    }
  }
  const bool masked = ap_any_key_valid(kmask, r, S);  // its block barrier also ends the staging of K and V
  const float scale = 1.0f / sqrtf((float)DH);
  if (active) {
    for (int jt = 0; jt < Sp / 16; ++jt) {
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
      const bool off = masked && j < S && !kmask[(long long)r * S + j];
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
    for (int c = c0; c < S; c += 4) mx = fmaxf(mx, row[c]);
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    float sum = 0.f;
    for (int c = c0; c < S; c += 4) {
      const float e = expf(row[c] - mx);
      row[c] = e;
      sum += e;
    }
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    const float inv = 1.0f / sum;
    float dsum = 0.f;
    for (int c = c0; c < S; c += 4) {
      const float p = row[c] * inv;
      row[c] = p;
      dsum += p * drow[c];
    }
    dsum += __shfl_xor(dsum, 1, 64);
    dsum += __shfl_xor(dsum, 2, 64);
    for (int c = c0; c < S; c += 4) drow[c] = row[c] * (drow[c] - dsum);
    for (int c = S + c0; c < Sp; c += 4) {
      row[c] = 0.f;
      drow[c] = 0.f;
    }
  }
  __syncthreads();
  if (active) {
    for (int rw = 0; rw < 16; ++rw) {
      const int i = i0 + rw;
      if (i >= L) break;
      for (int c = lane; c < Sp; c += 64) {
        Pg[(long long)i * Sp + c] = Pw[rw * LS + c];
        Sg[(long long)i * Sp + c] = Dw[rw * LS + c];
      }
    }
    f32x4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < Sp / 4; ++k) {
      const float a = Dw[lr * LS + k * 4 + lq];
      const float* kp = Ks + (k * 4 + lq) * LD + lr;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[ct] = mfma4(a, kp[ct * 16], acc[ct]);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = i0 + lq * 4 + g;
      if (i < L) {
        float* o = dq + ((long long)r * L + i) * D + h * DH + lr;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) o[ct * 16] = acc[ct][g] * scale;
      }
    }
  }
}

template <int DH>
__global__ __launch_bounds__(256) void attn_cross_bwd_kv_kernel(const float* __restrict__ q,
                                                                const float* __restrict__ dout,
                                                                float* __restrict__ dkv,
                                                                const float* __restrict__ scratch, int L, int S,
                                                                int Sp, int H) {
  extern __shared__ float sm[];
  constexpr int LD = DH + 4, CT = DH / 16;
  const int D = H * DH;
  const int r = blockIdx.x / H, h = blockIdx.x % H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  float* Qs = sm;
  float* Os = Qs + AP_QT * LD;
  const float* qb = q + (long long)r * L * D + h * DH;
  const float* dob = dout + (long long)r * L * D + h * DH;
  const float* Pg = scratch + (long long)blockIdx.x * 2 * L * Sp;
  const float* Sg = Pg + (long long)L * Sp;
  const int j0 = blockIdx.y * AP_QT + wave * 16;
  const bool active = j0 < S;  // wave-uniform; an idle wave still stages and keeps the barriers
  f32x4 av[CT], ak[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) av[ct] = ak[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ic = 0; ic < L; ic += AP_QT) {  // 64 queries at a time, ascending: a fixed summation order
    const int n = L - ic < AP_QT ? L - ic : AP_QT;
    const int np = (n + 15) / 16 * 16;
    if (ic) __syncthreads();  // the previous chunk has been read
    ap_stage<DH>(Qs, qb + (long long)ic * D, (long long)D, n, np);
    ap_stage<DH>(Os, dob + (long long)ic * D, (long long)D, n, np);
    __syncthreads();
    if (active)
      for (int k = 0; k < np / 4; ++k) {
        const int il = k * 4 + lq, i = ic + il;
        float ap = 0.f, as = 0.f;
        if (i < L) {  // column j0 + lr < Sp: inside the scratch row
          ap = Pg[(long long)i * Sp + j0 + lr];
          as = Sg[(long long)i * Sp + j0 + lr];
        }
        const float* op = Os + il * LD + lr;
        const float* qp = Qs + il * LD + lr;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          av[ct] = mfma4(ap, op[ct * 16], av[ct]);
          ak[ct] = mfma4(as, qp[ct * 16], ak[ct]);
        }
      }
  }
  if (!active) return;
  const float scale = 1.0f / sqrtf((float)DH);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int j = j0 + lq * 4 + g;
    if (j < S) {
      float* o = dkv + ((long long)r * S + j) * 2 * D + h * DH + lr;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        o[ct * 16] = ak[ct][g] * scale;
        o[D + ct * 16] = av[ct][g];
      }
    }
  }
}

extern "C" size_t vs_attn_cross_bwd_scratch_bytes(int R, int L, int S, int H) {
  if (R <= 0 || L <= 0 || S <= 0 || H <= 0) return 0;
  return (size_t)R * H * 2 * L * ap_lp(S) * sizeof(float);
}

template <int DH>
static int ax_bwd_launch(const float* q, const float* kv, const uint8_t* km, const float* dout, float* dq, float* dkv,
                         float* scratch, int R, int L, int S, int H, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    if (!ax_lds_attr((const void*)attn_cross_bwd_q_kernel<DH>) ||
        !ax_lds_attr((const void*)attn_cross_bwd_kv_kernel<DH>))
      return VS_ERR_LAUNCH;
    attr = true;
  }
  const int Sp = ap_lp(S);
  hipLaunchKernelGGL(attn_cross_bwd_q_kernel<DH>, dim3(R * H, (L + AP_QT - 1) / AP_QT), dim3(256), ap_bwd_smem(S, DH),
                     st, q, kv, km, dout, dq, scratch, L, S, Sp, H);
  hipLaunchKernelGGL(attn_cross_bwd_kv_kernel<DH>, dim3(R * H, (S + AP_QT - 1) / AP_QT), dim3(256), ax_bwd_kv_smem(DH),
                     st, q, dout, dkv, (const float*)scratch, L, S, Sp, H);
  return VS_OK;
}

extern "C" int vs_attn_cross_bwd(const float* q, const float* kv, const uint8_t* key_mask, const float* dout, float* dq,
                                 float* dkv, void* ws, size_t ws_bytes, int R, int L, int S, int H, int dh,
                                 void* stream) {
  VS_CHECK_ARG(q && kv && dout && dq && dkv && ws, "bad args");
  int rc = ax_check_shape(__func__, R, L, S, H, dh, true);
  if (rc != VS_OK) return rc;
  VS_CHECK_ARG(ws_bytes >= vs_attn_cross_bwd_scratch_bytes(R, L, S, H), "scratch too small");
  VS_CHECK_ARG((((uintptr_t)kv | (uintptr_t)q | (uintptr_t)dout) & 15) == 0 && ((uintptr_t)ws & 3) == 0,
               "q, kv and dout must be 16-byte aligned, the scratch 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  switch (dh) {
    case 16: rc = ax_bwd_launch<16>(q, kv, key_mask, dout, dq, dkv, (float*)ws, R, L, S, H, st); break;
    case 32: rc = ax_bwd_launch<32>(q, kv, key_mask, dout, dq, dkv, (float*)ws, R, L, S, H, st); break;
    case 64: rc = ax_bwd_launch<64>(q, kv, key_mask, dout, dq, dkv, (float*)ws, R, L, S, H, st); break;
    default: rc = ax_bwd_launch<128>(q, kv, key_mask, dout, dq, dkv, (float*)ws, R, L, S, H, st); break;
  }
  if (rc != VS_OK) return rc;
  VS_CHECK_LAUNCH();
  return VS_OK;
}

// 1 where the kernels above hold (L, S, dh) -- by the formulas their launchers check.
extern "C" int vs_attn_cross_fits(int L, int S, int dh, int backward) {
  if (L <= 0 || S <= 0 || !ap_dh_ok(dh) || (L + AP_QT - 1) / AP_QT > 65535) return 0;
  return (backward ? ap_bwd_smem(S, dh) : ap_fwd_smem(S, dh)) <= AP_LDS_MAX;
}

// ----------------------------------------------------------------------------
// One cached decode step: one query per (row, head) against the encoder K / V caches [rows, H, S, dh], written once per
// generation.  One wave per (row, head), four per block.  Scores: 16 lanes per key, each a float4 slice of the
// channels (a key's row is one contiguous read), four keys per pass, a 16-lane butterfly per key; a wave softmax with
// the lanes over the keys; p.V with the lanes over the channels (coalesced rows of V).  The scores live in the wave's
// LDS strip of S floats.  No host reads, every argument constant across replays of a captured step.
// ----------------------------------------------------------------------------
template <int DH>
__global__ __launch_bounds__(256) void attn_cross_decode_kernel(const float* __restrict__ q,
                                                                const float* __restrict__ kc,
                                                                const float* __restrict__ vc,
                                                                const uint8_t* __restrict__ kmask,
                                                                float* __restrict__ out, int n_pairs, int S, int H) {
  extern __shared__ float sm[];
  constexpr int V4 = DH / 4, NQ = (V4 + 15) / 16;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int pair = blockIdx.x * 4 + wave;
  if (pair >= n_pairs) return;  // wave-uniform; the kernel has no block barrier
  const int r = pair / H, h = pair - r * H;
  const int D = H * DH;
  float* sc = sm + wave * S;
  const float4* qp = (const float4*)(q + (long long)r * D + h * DH);
  const float* kp = kc + (long long)pair * S * DH;
  const float* vp = vc + (long long)pair * S * DH;
  const uint8_t* km = kmask ? kmask + (long long)r * S : nullptr;
  bool masked = false;  // ap_any_key_valid's rule, per wave
  if (km) {
    int any = 0;
    for (int j = lane; j < S; j += 64) any |= km[j];
    masked = __ballot(any != 0) != 0;
  }
  const int g = lane >> 4, sub = lane & 15;
  float4 qv[NQ];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    const int c = sub + 16 * n;
    qv[n] = c < V4 ? qp[c] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float scale = 1.0f / sqrtf((float)DH);
  for (int j0 = 0; j0 < S; j0 += 4) {
    const int j = j0 + g;
    float s = 0.f;
    if (j < S) {
      const float4* k4 = (const float4*)(kp + (long long)j * DH);
#pragma unroll
      for (int n = 0; n < NQ; ++n) {
        const int c = sub + 16 * n;
        if (c < V4) {
          const float4 k = k4[c];
          s += (qv[n].x * k.x + qv[n].y * k.y) + (qv[n].z * k.z + qv[n].w * k.w);
        }
      }
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    if (sub == 0 && j < S) sc[j] = (masked && !km[j]) ? -INFINITY : s * scale;
  }
  __builtin_amdgcn_wave_barrier();  // the wave's other lanes wrote what this lane reads
  float mx = -INFINITY;
  for (int j = lane; j < S; j += 64) mx = fmaxf(mx, sc[j]);
  mx = wave_reduce_max(mx);
  float sum = 0.f;
  for (int j = lane; j < S; j += 64) {
    const float e = expf(sc[j] - mx);
    sc[j] = e;
    sum += e;
  }
  sum = wave_reduce_sum(sum);
  const float inv = 1.0f / sum;
  __builtin_amdgcn_wave_barrier();
  float* o = out + (long long)r * D + h * DH;
  for (int c = lane; c < DH; c += 64) {
    float acc = 0.f;
    for (int j = 0; j < S; ++j) acc = fmaf(sc[j], vp[(long long)j * DH + c], acc);
    o[c] = acc * inv;
  }
}

extern "C" int vs_attn_cross_decode(const float* q, const float* kcache, const float* vcache, const uint8_t* key_mask,
                                    float* out, int rows, int S, int H, int dh, void* stream) {
  VS_CHECK_ARG(q && kcache && vcache && out && rows > 0 && S > 0 && H > 0, "bad args");
  VS_CHECK_ARG(ap_dh_ok(dh), "head width must be 16, 32, 64 or 128");
  VS_CHECK_ARG(S <= AX_DEC_SMAX, "source longer than the decode step's score strip (S <= 2048)");
  VS_CHECK_ARG((long long)rows * H <= 0x7fffffffLL, "too many (row, head) pairs");
  VS_CHECK_ARG((((uintptr_t)q | (uintptr_t)kcache) & 15) == 0, "q and the K cache must be 16-byte aligned");
  const int n = rows * H;
  const dim3 grid((n + 3) / 4), block(256);
  const size_t smem = (size_t)4 * S * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  switch (dh) {
    case 16: hipLaunchKernelGGL(attn_cross_decode_kernel<16>, grid, block, smem, st, q, kcache, vcache, key_mask, out, n, S, H); break;
    case 32: hipLaunchKernelGGL(attn_cross_decode_kernel<32>, grid, block, smem, st, q, kcache, vcache, key_mask, out, n, S, H); break;
    case 64: hipLaunchKernelGGL(attn_cross_decode_kernel<64>, grid, block, smem, st, q, kcache, vcache, key_mask, out, n, S, H); break;
    default: hipLaunchKernelGGL(attn_cross_decode_kernel<128>, grid, block, smem, st, q, kcache, vcache, key_mask, out, n, S, H); break;
  }
  VS_CHECK_LAUNCH();
  return VS_OK;
}

// ----------------------------------------------------------------------------
// kv [R*S, 2D] (k | v, heads merged) -> the decode step's caches K, V [R, H, S, dh]; once per layer and generation
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_cross_kv_split_kernel(const float4* __restrict__ kv,
                                                                  float* __restrict__ kc, float* __restrict__ vc,
                                                                  long long n4, int S, int H, int dh) {
  const int D = H * dh, W4 = 2 * D / 4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const long long row = i / W4;
    int col = (int)(i - row * W4) * 4;
    const long long r = row / S;
    const int s = (int)(row - r * S);
    float* dst = kc;
    if (col >= D) {
      col -= D;
      dst = vc;
    }
    const int h = col / dh, c = col - h * dh;
    *(float4*)(dst + (((r * H + h) * S + s) * (long long)dh + c)) = kv[i];
  }
}

extern "C" int vs_attn_cross_kv_split(const float* kv, float* kcache, float* vcache, int R, int S, int H, int dh,
                                      void* stream) {
  VS_CHECK_ARG(kv && kcache && vcache && R > 0 && S > 0 && H > 0, "bad args");
  VS_CHECK_ARG(ap_dh_ok(dh), "head width must be 16, 32, 64 or 128");
  VS_CHECK_ARG((((uintptr_t)kv | (uintptr_t)kcache | (uintptr_t)vcache) & 15) == 0, "buffers must be 16-byte aligned");
  const long long n4 = (long long)R * S * 2 * H * dh / 4;
  long long g = (n4 + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(attn_cross_kv_split_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                     (const float4*)kv, kcache, vcache, n4, S, H, dh);
  VS_CHECK_LAUNCH();
  return VS_OK;
}
