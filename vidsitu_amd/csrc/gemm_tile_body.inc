// Body of gemm_nt_kernel / gemm_ld_kernel (gemm_nt.hip): in scope are the template parameters Op, BM, BN, KVEC, the
// kernel arguments x, w, bias, res, y, M, N, K, act, kts and the leading dimensions lda, ldb of K-strided operands.
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
  // strided loader mapping: first row and k-pair of this thread in a 64-row pass (comment at GemmBf16T)
  const int tr = 4 * (8 * (wave & 1) + 4 * (lane >> 5) + (lane & 3)), tkp = 8 * (wave >> 1) + ((lane >> 2) & 7);
  // 4 consecutive rows of a [K][rows] operand at one k, as branch-free and raw as ld4: a lane (on the scalar path, an
  // element) out of range reads element 0, and tstore zeroes it.
  auto ldt = [&](const float* base, int row, int rows, int ld, int k, int bit) __attribute__((always_inline)) {
    const bool ok = row < rows && k < K;
    okmask = ok ? (okmask | (1u << bit)) : (okmask & ~(1u << bit));
    const long long o = ok ? (long long)k * ld + row : 0;
    if constexpr (kvec) return *(const float4*)(base + o);
    float4 v;
    v.x = base[o];
    v.y = base[ok && row + 1 < rows ? o + 1 : 0];
    v.z = base[ok && row + 2 < rows ? o + 2 : 0];
    v.w = base[ok && row + 3 < rows ? o + 3 : 0];
    return v;
  };
  auto gload = [&](int k0) __attribute__((always_inline)) {
    if constexpr (Op::A_T) {  // registers 2j, 2j + 1: k even, k odd of 64-row pass j
#pragma unroll
      for (int i = 0; i < PA; ++i) ra[i] = ldt(x, m0 + tr + 64 * (i >> 1), M, lda, k0 + 2 * tkp + (i & 1), i);
    } else {
#pragma unroll
      for (int i = 0; i < PA; ++i) ra[i] = ld4(x, m0 + lr + 32 * i, M, k0 + lc * 4, i);
    }
    if constexpr (Op::B_T) {
#pragma unroll
      for (int i = 0; i < PB; ++i) rb[i] = ldt(w, n0 + tr + 64 * (i >> 1), N, ldb, k0 + 2 * tkp + (i & 1), PA + i);
    } else {
#pragma unroll
      for (int i = 0; i < PB; ++i) rb[i] = ld4(w, n0 + lr + 32 * i, N, k0 + lc * 4, PA + i);
    }
  };
  // tile store of a strided operand: rows tr .. tr + 3 of each 64-row pass at k-pair tkp, one dword per row
  auto tstore = [&](elem* tile, const float4* r, int passes, int row0, int rows, int bit0)
                    __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < passes; i += 2) {
      const bool ok0 = (okmask >> (bit0 + i)) & 1, ok1 = (okmask >> (bit0 + i + 1)) & 1;
      const float lo[4] = {r[i].x, r[i].y, r[i].z, r[i].w}, hi[4] = {r[i + 1].x, r[i + 1].y, r[i + 1].z, r[i + 1].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = tr + 32 * i + e;
        const bool in = kvec || row0 + row < rows;  // 16-byte loads: a row quad is inside or outside as a whole
        *(uint32_t*)&tile[row * LD + 2 * tkp] = pack2_bf16(ok0 && in ? lo[e] : 0.f, ok1 && in ? hi[e] : 0.f);
      }
    }
  };
  // The unconverted stores stand here and not behind a function of the policy: routed through one (member, lambda,
  // by value or by reference), the fp32 128x128 kernel gets another register assignment with the same instructions
  // and runs 3 % (N = 3072) to 12 % (N = 4096) slower at 3000 x N x 1024 (profiles/gemm_unify.txt).
  auto sstore = [&](int buf) __attribute__((always_inline)) {
    if constexpr (Op::A_T) tstore(As[buf], ra, PA, m0, M, 0);
#pragma unroll
    for (int i = 0; i < (Op::A_T ? 0 : PA); ++i) {
      elem* a = &As[buf][(lr + 32 * i) * LD + lc * 4];
      const bool ok = (okmask >> i) & 1;
      if constexpr (Op::PACKED) Op::store4(a, ra[i], ok);
      else {
        a[0] = ok ? ra[i].x : 0.f; a[1] = ok ? ra[i].y : 0.f; a[2] = ok ? ra[i].z : 0.f; a[3] = ok ? ra[i].w : 0.f;
      }
    }
    if constexpr (Op::B_T) tstore(Bs[buf], rb, PB, n0, N, PA);
#pragma unroll
    for (int i = 0; i < (Op::B_T ? 0 : PB); ++i) {
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
