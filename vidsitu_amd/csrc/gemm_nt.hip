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
// stores the four floats of a loader lane (otherwise the kernel stores them as they are).  A_T / B_T: that operand is
// stored [K][rows] ("K-strided": rows contiguous, K the slow axis) and takes the strided loader (GemmBf16T only).
//
// fp32 operands, the reference's arithmetic (v_mfma_f32_32x32x2_f32, 157 TFLOP/s dense on MI355X).  Odd pitch (33
// floats): the fragment read of a 32x32x2 MFMA (lane l: row l&31, k = l>>5) is then conflict free.
struct GemmF32 {
  typedef float elem, frag;
  static constexpr int LD = 33, KSTEP = 2, ALIGN = 4;
  static constexpr bool PACKED = false, A_T = false, B_T = false;
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
  static constexpr bool PACKED = true, A_T = false, B_T = false;
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

// The same tiles from K-strided operands: the two products of a dense layer's backward without a transposed copy,
// dx = dy . W (B = W[out][in] strided) and dW = dy^T . x (A = dy[T][out] and B = x[T][in] both strided, K = T).
// The strided loader reads along the row axis: a thread owns 4 consecutive rows at the k-pair (2 kp, 2 kp + 1) -- two
// float4 loads, or 8 scalar ones -- and stores each row's pair as one dword, pack2_bf16(k even, k odd): the rounding
// of store4.  The tile it leaves is byte for byte the tile the K-contiguous loader leaves for the transposed copy, so
// everything behind the tile store is shared.  Thread -> (row quad rq of 16, k-pair kp of 16) of a 64-row pass:
// rq = 8 * (wave & 1) + 4 * (lane >> 5) + (lane & 3), kp = 8 * (wave >> 1) + ((lane >> 2) & 7).  A wave's load is 8
// segments of 128 contiguous bytes (8 row quads at each of 8 values of k).  ds_write_b32 is served in two groups of
// 32 lanes on 32 dword banks; row r, pair kp sits at dword 20 r + kp, so the 4 row quads x 8 pairs of a group fall on
// 16 banks with two addresses each: 2-way, which a ds_write_b32 hides behind its own 4 issue cycles (a store conflict
// costs time only once the LDS-array cycles exceed them; 16 row quads at 2 pairs, the mapping that loads 256-byte
// segments, is 8-way).  tools/probes/gemm_bf16_lds_sim.py counts it: 2.00 array cycles per group in every wave.
// (The compiler pairs the stores of two rows of a quad into one ds_write2_b32: the same two accesses.)
template <bool AT, bool BT>
struct GemmBf16T : GemmBf16 {
  static constexpr bool A_T = AT, B_T = BT;
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
// KVEC: every operand takes 16-byte loads (K-contiguous: K % 4 == 0; K-strided: row count and leading dimension
// % 4 == 0; bases aligned).
template <class Op, int BM, int BN, bool KVEC>  // 128x128 (2x2 MFMA tiles per wave) or 64x64 (one per wave)
__global__ __launch_bounds__(256) void gemm_nt_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, const float* res, float* y,
                                                      int M, int N, int K, int act, int kts) {
  constexpr int lda = 0, ldb = 0;  // no strided operand
#include "gemm_tile_body.inc"
}

// The strided forms carry the leading dimension of each strided operand: the row count of the array it is a row range
// of (dqkv[T][3D] feeds three weight gradients of D rows each).  The kernel text is the one above, and is included
// rather than called: behind a function the fp32 kernels get another register assignment (profiles/gemm_unify.txt),
// and two more kernel arguments would move the ones the runtime appends.
template <class Op, int BM, int BN, bool KVEC>
__global__ __launch_bounds__(256) void gemm_ld_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, const float* res, float* y,
                                                      int M, int N, int K, int act, int kts, int lda, int ldb) {
#include "gemm_tile_body.inc"
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
                           const float* res, float* y, int M, int N, int K, int act, int kts, int lda, int ldb) {
  if constexpr (Op::A_T || Op::B_T) {
    if (kv)
      hipLaunchKernelGGL((gemm_ld_kernel<Op, BM, BN, true>), grid, dim3(256), 0, st, x, w, b, res, y, M, N, K, act,
                         kts, lda, ldb);
    else
      hipLaunchKernelGGL((gemm_ld_kernel<Op, BM, BN, false>), grid, dim3(256), 0, st, x, w, b, res, y, M, N, K, act,
                         kts, lda, ldb);
  } else if (kv)
    hipLaunchKernelGGL((gemm_nt_kernel<Op, BM, BN, true>), grid, dim3(256), 0, st, x, w, b, res, y, M, N, K, act, kts);
  else
    hipLaunchKernelGGL((gemm_nt_kernel<Op, BM, BN, false>), grid, dim3(256), 0, st, x, w, b, res, y, M, N, K, act, kts);
}

// Tile choice and split-K of both arms, every M >= 1.  A missing or short workspace runs the unsplit 64x64 kernel.
// kv: every operand can take 16-byte loads (the caller knows the operand forms).
template <class Op>
static int gemm_nt_mfma(const float* x, const float* w, const float* b, const float* res, float* y, int M, int N,
                        int K, int act, hipStream_t st, void* workspace, size_t ws_bytes, bool kv, int lda = 0,
                        int ldb = 0) {
  // fewer than one 128x128 tile per CU: 64x64 tiles (4x the blocks) keep the chip busy
  const long long t128 = (long long)((M + 127) / 128) * ((N + 127) / 128);
  const dim3 g64((N + 63) / 64, (M + 63) / 64);
  const int S = workspace && t128 < 256 ? gemm_split(M, N, K) : 1;
  if (t128 >= 256) {
    gemm_nt_launch<Op, 128, 128>(kv, dim3((N + 127) / 128, (M + 127) / 128), st, x, w, b, res, y, M, N, K, act, 0,
                                 lda, ldb);
  } else if (S > 1 && ws_bytes >= (size_t)S * M * N * sizeof(float)) {
    const int nk = (K + GM_BK - 1) / GM_BK;
    const int kts = (nk + S - 1) / S;
    const int Se = (nk + kts - 1) / kts;  // slices that own at least one k-tile
    gemm_nt_launch<Op, 64, 64>(kv, dim3(g64.x, g64.y, Se), st, x, w, nullptr, nullptr, (float*)workspace, M, N, K, 0,
                               kts, lda, ldb);
    const long long MN = (long long)M * N;
    const unsigned grid = MN > 4096 * 256 ? 4096 : (unsigned)((MN + 255) / 256);
    hipLaunchKernelGGL(gemm_splitk_reduce_kernel, dim3(grid), dim3(256), 0, st, (const float*)workspace, b, res, y, MN,
                       N, Se, act);
  } else {
    gemm_nt_launch<Op, 64, 64>(kv, g64, st, x, w, b, res, y, M, N, K, act, 0, lda, ldb);
  }
  VS_CHECK_LAUNCH();
  return VS_OK;
}

// both operands K-contiguous
template <class Op>
static int gemm_nt_mfma(const float* x, const float* w, const float* b, const float* res, float* y, int M, int N,
                        int K, int act, hipStream_t st, void* workspace, size_t ws_bytes) {
  const bool kv = (K & 3) == 0 && ((((uintptr_t)x | (uintptr_t)w)) & 15) == 0;
  return gemm_nt_mfma<Op>(x, w, b, res, y, M, N, K, act, st, workspace, ws_bytes, kv);
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

/* vs_gemm_nt_bf16_ws with either operand K-strided, as a row range of an array of lda / ldb rows (vidsitu_hip.h). */
extern "C" int vs_gemm_bf16_ld_ws(const float* a, const float* b, const float* bias, const float* res, float* y, int M,
                                  int N, int K, int a_kstrided, int b_kstrided, int lda, int ldb, int act,
                                  void* workspace, size_t ws_bytes, void* stream) {
  VS_CHECK_ARG(a && b && y && M > 0 && N > 0 && K > 0, "bad args");
  VS_CHECK_ARG(act >= 0 && act <= 2, "act must be 0 (none), 1 (relu) or 2 (gelu_new)");
  VS_CHECK_ARG((a_kstrided | b_kstrided | 1) == 1, "a_kstrided and b_kstrided must be 0 or 1");
  VS_CHECK_ARG((!a_kstrided || lda >= M) && (!b_kstrided || ldb >= N),
               "the leading dimension of a K-strided operand is at least its row count");
  const size_t need = gemm_workspace_bytes(M, N, K);
  VS_CHECK_ARG(!need || (workspace && ws_bytes >= need), "workspace shorter than vs_gemm_nt_bf16_workspace_bytes");
  hipStream_t st = (hipStream_t)stream;
  if (!a_kstrided && !b_kstrided)
    return gemm_nt_mfma<GemmBf16>(a, b, bias, res, y, M, N, K, act, st, workspace, ws_bytes);
  // 16-byte loads run along an operand's contiguous axis: K, or the rows of a strided operand (whole row quads)
  const bool kv = ((((uintptr_t)a | (uintptr_t)b)) & 15) == 0 && ((a_kstrided ? M | lda : K) & 3) == 0 &&
                  ((b_kstrided ? N | ldb : K) & 3) == 0;
  if (!a_kstrided)
    return gemm_nt_mfma<GemmBf16T<false, true>>(a, b, bias, res, y, M, N, K, act, st, workspace, ws_bytes, kv, 0, ldb);
  if (!b_kstrided)
    return gemm_nt_mfma<GemmBf16T<true, false>>(a, b, bias, res, y, M, N, K, act, st, workspace, ws_bytes, kv, lda, 0);
  return gemm_nt_mfma<GemmBf16T<true, true>>(a, b, bias, res, y, M, N, K, act, st, workspace, ws_bytes, kv, lda, ldb);
}

/* The same with whole arrays: lda = M, ldb = N. */
extern "C" int vs_gemm_bf16_ws(const float* a, const float* b, const float* bias, const float* res, float* y, int M,
                               int N, int K, int a_kstrided, int b_kstrided, int act, void* workspace,
                               size_t ws_bytes, void* stream) {
  return vs_gemm_bf16_ld_ws(a, b, bias, res, y, M, N, K, a_kstrided, b_kstrided, M, N, act, workspace, ws_bytes,
                            stream);
}
