// y[M,N] = act(x[M,K] . w[N,K]^T + b) + res on the matrix cores (gfx950), "NT": both operands K-contiguous.  The dense
// projection of every transformer host above 64 rows (up to 64, txenc_ops.hip streams the weights); fp32 in memory, in
// the accumulators and in the epilogue.  One kernel and one dispatcher behind two operand policies.
// 128x128x32 (or 64x64x32) tile, 4 waves as 2x2, each wave a block of 32x32 MFMA accumulators.  LDS rows are K-major,
// element type and pitch the policy's.  Register-staged double buffer.
#include <math.h>

#include "common.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;
#define GM_BK 32

// An operand policy: LDS element and MFMA fragment type, row pitch LD (elements), k extent KSTEP of one MFMA, LDS
// alignment, frag_k (k offset of the fragment of lane >> 5), load (one fragment), mfma, and PACKED: store4 converts and
// stores the four floats of a loader lane (otherwise the kernel stores them as they are).
//
// fp32 operands, the reference's arithmetic (v_mfma_f32_32x32x2_f32, 157 TFLOP/s dense on MI355X).  Odd pitch (33
// floats): the fragment read of a 32x32x2 MFMA (lane l: row l&31, k = l>>5) is then conflict free.
struct GemmF32 {
  typedef float elem, frag;
  static constexpr int LD = 33, KSTEP = 2, ALIGN = 4;
  static constexpr bool PACKED = false;
  static __device__ __forceinline__ int frag_k(int fk) { return fk; }
  static __device__ __forceinline__ float load(const float* p) { return *p; }
  static __device__ __forceinline__ f32x16 mfma(float a, float b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
  }
};

// bf16 operands (opt-in mixed precision of the whole-sequence passes): x and w stay fp32 in memory; store4 rounds each
// element to bf16 (nearest, ties to even: v_cvt_pk_bf16_f32) where it writes the tile to LDS, and the main loop runs
// v_mfma_f32_32x32x16_bf16 with fp32 accumulators.  bf16 x bf16 products are exact in fp32, so the result differs from
// an fp32 GEMM over the rounded operands by summation order only.
// LDS rows are K-major bf16 with a pitch of 40 elements = 80 bytes (the 64 bytes of a k-tile + one 16-byte slot).
// A lane's fragment (row lane & 31, k = 16 * step + 8 * (lane >> 5) .. + 7) is one ds_read_b128 at 16-byte slot
// 5 * row + 2 * step + (lane >> 5).  ds_read_b128 is served in four groups of 16 lanes (MI355X: {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same + 32); the rows of a group cover every residue mod 16 once and share lane >> 5,
// and 5 is odd, so its 16 slots are the 16 distinct slots of the 256-byte bank row: conflict free
// (tools/probes/gemm_bf16_lds_sim.py counts it, and the 2-way conflicts the 8-byte tile stores keep).
struct GemmBf16 {
  typedef uint16_t elem;
  typedef bf16x8 frag;
  static constexpr int LD = 40, KSTEP = 16, ALIGN = 16;
  static constexpr bool PACKED = true;
  static __device__ __forceinline__ void store4(uint16_t* dst, const float4& r, bool ok) {
    uint2 v;
    v.x = pack2_bf16(ok ? r.x : 0.f, ok ? r.y : 0.f);
    v.y = pack2_bf16(ok ? r.z : 0.f, ok ? r.w : 0.f);
    *(uint2*)dst = v;
  }
  static __device__ __forceinline__ int frag_k(int fk) { return fk * 8; }
  static __device__ __forceinline__ bf16x8 load(const uint16_t* p) { return *(const bf16x8*)p; }
  static __device__ __forceinline__ f32x16 mfma(const bf16x8& a, const bf16x8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};

// Epilogue of one wave's MR x NR block of 32x32 accumulators (the D layout of a 32x32 MFMA does not depend on the
// operand type): col = lane & 31, row = 8*(e/4) + 4*(lane>>5) + (e&3).
// raw: a split-K slice stores its partial tile as it is (y already points at the slice's slab).
template <int BM, int BN>
__device__ __forceinline__ void gemm_tile_epilogue(const f32x16 (&acc)[BM / 64][BN / 64], const float* __restrict__ bias,
                                                   const float* res, float* y, int M, int N, int mw, int nw, int lane,
                                                   int act, bool raw) {
#pragma unroll
  for (int a = 0; a < BM / 64; ++a)
#pragma unroll
    for (int b = 0; b < BN / 64; ++b) {
      const int n = nw + b * 32 + (lane & 31);
      if (n >= N) continue;
      if (raw) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = mw + a * 32 + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
          if (m < M) y[(long long)m * N + n] = acc[a][b][e];
        }
        continue;
      }
      const float bvv = bias ? bias[n] : 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = mw + a * 32 + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
        if (m < M) {
          float v = acc[a][b][e] + bvv;
          if (act == 1) v = fmaxf(v, 0.f);
          else if (act == 2) v = gelu_new_f(v);
          if (res) v += res[(long long)m * N + n];
          y[(long long)m * N + n] = v;
        }
      }
    }
}

// Split-K (gridDim.z = S > 1): slice z covers k-tiles [z * kts, (z + 1) * kts) and stores its raw partial
// tile into slab z of `y` (M * N floats each); gemm_splitk_reduce_kernel adds the slabs in slice order and
// applies the epilogue.  Layers with few output tiles (600 x 1024: 160 tiles of 64 x 64 for 256 CUs) then
// run 3-4 blocks per CU and overlap each other's memory latency.
template <class Op, int BM, int BN, bool KVEC>  // 128x128 (2x2 MFMA tiles per wave) or 64x64 (one per wave); K % 4 == 0
__global__ __launch_bounds__(256) void gemm_nt_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, const float* res, float* y,
                                                      int M, int N, int K, int act, int kts) {
  typedef typename Op::elem elem;
  constexpr int LD = Op::LD;
  constexpr int MR = BM / 64, NR = BN / 64;  // 32x32 accumulators per wave
  constexpr int PA = BM / 32, PB = BN / 32;  // loader passes (32 rows each)
  __shared__ __attribute__((aligned(Op::ALIGN))) elem As[2][BM * LD];
  __shared__ __attribute__((aligned(Op::ALIGN))) elem Bs[2][BN * LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  // loader mapping: 8 float4 per 32-float row, 32 rows per pass
  const int lc = tid & 7, lr = tid >> 3;
  constexpr bool kvec = KVEC;  // compile time: a runtime flag put every load behind a branch (and a wait)
  float4 ra[PA], rb[PB];

  // Loads are branch-free (a load inside `if (ok)` sits in its own basic block behind its own wait: the 8
  // loads of a k-tile were 8 serialised round trips) and RAW: out-of-range lanes read element 0 and are
  // zeroed only when the tile is written to LDS, so nothing touches the loaded registers -- and no wait is
  // placed -- before the MFMAs of the current tile have been issued.
  unsigned okmask = 0;
  auto ld4 = [&](const float* base, int row, int rows, int k, int bit) __attribute__((always_inline)) {
    const bool ok = row < rows && k < K;
    okmask = ok ? (okmask | (1u << bit)) : (okmask & ~(1u << bit));
    if constexpr (kvec) return *(const float4*)(base + (ok ? (long long)row * K + k : 0));
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
      const float* s = base + (long long)row * K + k;
      v.x = s[0]; if (k + 1 < K) v.y = s[1]; if (k + 2 < K) v.z = s[2]; if (k + 3 < K) v.w = s[3];
    }
    return v;
  };
  auto gload = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < PA; ++i) ra[i] = ld4(x, m0 + lr + 32 * i, M, k0 + lc * 4, i);
#pragma unroll
    for (int i = 0; i < PB; ++i) rb[i] = ld4(w, n0 + lr + 32 * i, N, k0 + lc * 4, PA + i);
  };
  // The unconverted stores stand here and not behind a function of the policy: routed through one (member, lambda,
  // by value or by reference), the fp32 128x128 kernel gets another register assignment with the same instructions
  // and runs 3 % (N = 3072) to 12 % (N = 4096) slower at 3000 x N x 1024 (profiles/gemm_unify.txt).
  auto sstore = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < PA; ++i) {
      elem* a = &As[buf][(lr + 32 * i) * LD + lc * 4];
      const bool ok = (okmask >> i) & 1;
      if constexpr (Op::PACKED) Op::store4(a, ra[i], ok);
      else {
        a[0] = ok ? ra[i].x : 0.f; a[1] = ok ? ra[i].y : 0.f; a[2] = ok ? ra[i].z : 0.f; a[3] = ok ? ra[i].w : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      elem* b = &Bs[buf][(lr + 32 * i) * LD + lc * 4];
      const bool ok = (okmask >> (PA + i)) & 1;
      if constexpr (Op::PACKED) Op::store4(b, rb[i], ok);
      else {
        b[0] = ok ? rb[i].x : 0.f; b[1] = ok ? rb[i].y : 0.f; b[2] = ok ? rb[i].z : 0.f; b[3] = ok ? rb[i].w : 0.f;
      }
    }
  };

  f32x16 acc[MR][NR] = {};

  const int fr = lane & 31, fk = lane >> 5;
  const int nk_all = (K + GM_BK - 1) / GM_BK;
  const bool split = gridDim.z > 1;
  const int kt0 = split ? blockIdx.z * kts : 0;
  const int nk = split ? min(nk_all, kt0 + kts) : nk_all;
  if (split) y += (long long)blockIdx.z * M * N;
  gload(kt0 * GM_BK);
  sstore(kt0 & 1);
  __syncthreads();
  for (int kt = kt0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) gload((kt + 1) * GM_BK);
    const elem* A = &As[cur][(wm * (BM / 2) + fr) * LD + Op::frag_k(fk)];
    const elem* B = &Bs[cur][(wn * (BN / 2) + fr) * LD + Op::frag_k(fk)];
#pragma unroll
    for (int ks = 0; ks < GM_BK; ks += Op::KSTEP) {
      typename Op::frag av[MR], bv[NR];
#pragma unroll
      for (int a = 0; a < MR; ++a) av[a] = Op::load(A + a * 32 * LD + ks);
#pragma unroll
      for (int b = 0; b < NR; ++b) bv[b] = Op::load(B + b * 32 * LD + ks);
#pragma unroll
      for (int a = 0; a < MR; ++a)
#pragma unroll
        for (int b = 0; b < NR; ++b) acc[a][b] = Op::mfma(av[a], bv[b], acc[a][b]);
    }
    if (kt + 1 < nk) sstore(cur ^ 1);
    __syncthreads();
  }
  gemm_tile_epilogue<BM, BN>(acc, bias, res, y, M, N, m0 + wm * (BM / 2), n0 + wn * (BN / 2), lane, act, split);
}

__global__ void gemm_splitk_reduce_kernel(const float* slabs, const float* bias, const float* res, float* y,
                                          long long MN, int N, int S, int act) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < MN; i += (long long)gridDim.x * blockDim.x) {
    float v = slabs[i];
    for (int s2 = 1; s2 < S; ++s2) v += slabs[(long long)s2 * MN + i];
    if (bias) v += bias[i % N];
    if (act == 1) v = fmaxf(v, 0.f);
    else if (act == 2) v = gelu_new_f(v);
    if (res) v += res[i];
    y[i] = v;
  }
}

// K slices for a GEMM with few output tiles: about 700 blocks, at least 4 k-tiles (128 floats) per slice
static int gemm_split(int M, int N, int K) {
  const long long t128 = (long long)((M + 127) / 128) * ((N + 127) / 128);
  if (t128 >= 256) return 1;
  const long long t64 = (long long)((M + 63) / 64) * ((N + 63) / 64);
  const int nk = (K + GM_BK - 1) / GM_BK;
  int S = (int)(704 / t64);
  if (S > nk / 4) S = nk / 4;
  if (S > 16) S = 16;
  return S < 2 ? 1 : S;
}

static size_t gemm_workspace_bytes(int M, int N, int K) {
  const int S = gemm_split(M, N, K);
  return S > 1 ? (size_t)S * M * N * sizeof(float) : 0;
}

template <class Op, int BM, int BN>
static void gemm_nt_launch(bool kv, dim3 grid, hipStream_t st, const float* x, const float* w, const float* b,
                           const float* res, float* y, int M, int N, int K, int act, int kts) {
  if (kv)
    hipLaunchKernelGGL((gemm_nt_kernel<Op, BM, BN, true>), grid, dim3(256), 0, st, x, w, b, res, y, M, N, K, act, kts);
  else
    hipLaunchKernelGGL((gemm_nt_kernel<Op, BM, BN, false>), grid, dim3(256), 0, st, x, w, b, res, y, M, N, K, act, kts);
}

// Tile choice and split-K of both arms, every M >= 1.  A missing or short workspace runs the unsplit 64x64 kernel.
template <class Op>
static int gemm_nt_mfma(const float* x, const float* w, const float* b, const float* res, float* y, int M, int N,
                        int K, int act, hipStream_t st, void* workspace, size_t ws_bytes) {
  // fewer than one 128x128 tile per CU: 64x64 tiles (4x the blocks) keep the chip busy
  const long long t128 = (long long)((M + 127) / 128) * ((N + 127) / 128);
  const bool kv = (K & 3) == 0 && ((((uintptr_t)x | (uintptr_t)w)) & 15) == 0;
  const dim3 g64((N + 63) / 64, (M + 63) / 64);
  const int S = workspace && t128 < 256 ? gemm_split(M, N, K) : 1;
  if (t128 >= 256) {
    gemm_nt_launch<Op, 128, 128>(kv, dim3((N + 127) / 128, (M + 127) / 128), st, x, w, b, res, y, M, N, K, act, 0);
  } else if (S > 1 && ws_bytes >= (size_t)S * M * N * sizeof(float)) {
    const int nk = (K + GM_BK - 1) / GM_BK;
    const int kts = (nk + S - 1) / S;
    const int Se = (nk + kts - 1) / kts;  // slices that own at least one k-tile
    gemm_nt_launch<Op, 64, 64>(kv, dim3(g64.x, g64.y, Se), st, x, w, nullptr, nullptr, (float*)workspace, M, N, K, 0,
                               kts);
    const long long MN = (long long)M * N;
    const unsigned grid = MN > 4096 * 256 ? 4096 : (unsigned)((MN + 255) / 256);
    hipLaunchKernelGGL(gemm_splitk_reduce_kernel, dim3(grid), dim3(256), 0, st, (const float*)workspace, b, res, y, MN,
                       N, Se, act);
  } else {
    gemm_nt_launch<Op, 64, 64>(kv, g64, st, x, w, b, res, y, M, N, K, act, 0);
  }
  VS_CHECK_LAUNCH();
  return VS_OK;
}

// the fp32 arm above 64 rows, for vs_gemm_nt_f32 (txenc_ops.hip)
int vs_gemm_nt_f32_mfma(const float* x, const float* w, const float* b, const float* res, float* y, int M, int N,
                        int K, int act, hipStream_t st, void* ws, size_t ws_bytes) {
  return gemm_nt_mfma<GemmF32>(x, w, b, res, y, M, N, K, act, st, ws, ws_bytes);
}

// 0 = not needed; rows up to 64 never reach the MFMA kernel
extern "C" size_t vs_gemm_nt_f32_workspace_bytes(int M, int N, int K) {
  return M <= 64 ? 0 : gemm_workspace_bytes(M, N, K);
}

extern "C" size_t vs_gemm_nt_bf16_workspace_bytes(int M, int N, int K) {
  return M <= 0 || N <= 0 || K <= 0 ? 0 : gemm_workspace_bytes(M, N, K);
}

/* vs_gemm_nt_f32 with a split-K workspace (vs_gemm_nt_f32_workspace_bytes(M, N, K)). */
extern "C" int vs_gemm_nt_f32_ws(const float* x, const float* w, const float* b, const float* res, float* y,
                                 int M, int N, int K, int act, void* workspace, size_t ws_bytes, void* stream) {
  VS_CHECK_ARG(x && w && y && M > 0 && N > 0 && K > 0, "bad args");
  VS_CHECK_ARG(act >= 0 && act <= 2, "act must be 0 (none), 1 (relu) or 2 (gelu_new)");
  if (M <= 64 || !workspace) return vs_gemm_nt_f32(x, w, b, res, y, M, N, K, act, stream);
  return gemm_nt_mfma<GemmF32>(x, w, b, res, y, M, N, K, act, (hipStream_t)stream, workspace, ws_bytes);
}

/* y = act(bf16(x) . bf16(w)^T + b) + res with fp32 accumulation, every M >= 1. */
extern "C" int vs_gemm_nt_bf16_ws(const float* x, const float* w, const float* b, const float* res, float* y,
                                  int M, int N, int K, int act, void* workspace, size_t ws_bytes, void* stream) {
  VS_CHECK_ARG(x && w && y && M > 0 && N > 0 && K > 0, "bad args");
  VS_CHECK_ARG(act >= 0 && act <= 2, "act must be 0 (none), 1 (relu) or 2 (gelu_new)");
  return gemm_nt_mfma<GemmBf16>(x, w, b, res, y, M, N, K, act, (hipStream_t)stream, workspace, ws_bytes);
}
