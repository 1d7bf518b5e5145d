// Fused frame ingest (both halves in ONE launch): decoded uint8 frames at their source
// size -> Pillow's two-pass bicubic resize (resize_u8.hip: same tables, same integer arithmetic, clip after EACH
// pass) -> (x / 255 - mean) / std -> bf16 -> the packed channels-last stem input of the fast pathway and, for
// the frames the slow index selects, of the slow pathway.  Bit for bit what vs_resize_bicubic_u8 followed by one
// vs_frames_u8_pack per pathway writes; the resized uint8 frames never reach memory.
//
// One block (256 threads) per (frame, band of output rows):
//   1. horizontal pass of the band's source rows y_lo .. y_hi into an LDS tile [rows][pitch] of uint8 RGB.  One
//      thread per (row, output column); the window is read 4 taps = 12 bytes at a time (the taps of a window are
//      contiguous bytes of one source row; the loads are unaligned by construction), the 0..3 taps left over by bytes;
//   2. vertical pass out of the tile.  The vertical pass is independent per BYTE column, so one thread takes 12
//      consecutive bytes = 4 pixels (three 4-byte LDS reads per tap instead of twelve 1-byte ones); the band's
//      vertical weights sit in LDS;
//   3. normalise + round: a function of (byte value, channel) only, so the block computes the 3 x 256 bf16 results
//      once (the two IEEE divisions per byte of frames_u8_pack_kernel, same expression, same compile flags) and
//      step 3 is a table look-up; 8 (Cpad 4) or 16 (Cpad 8) bytes per pixel go out per store.
// A pass whose size does not change is skipped as in Pillow (template flags): the tile then holds source bytes
// (no horizontal pass) and / or exactly the band's rows (no vertical pass).
#include "common.h"
#include <math.h>

#define IG_PRECISION_BITS (32 - 8 - 2)
#define IG_THREADS 256
#define IG_LUT_BYTES (3 * 256 * 2)
#define IG_MAX_BAND 32

// Pillow's window of output index xx (precompute_coeffs; the same expressions as vs_resize_coeffs)
static inline void ig_window(int in_size, int out_size, int xx, int* first, int* count) {
  const double scale = (double)in_size / out_size;
  const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  *first = xmin;
  *count = xmax - xmin;
}

static inline int ig_pitch(int Wo) { return (Wo + 3) / 4 * 12; }

// LDS bytes of a block that produces `band` output rows from a tile of `rows` rows
static inline size_t ig_lds_bytes(int band, int rows, int Wo, int ksize_v) {
  return (size_t)IG_LUT_BYTES + (size_t)band * (ksize_v + 2) * 4 + (size_t)rows * ig_pitch(Wo);
}

extern "C" int vs_ingest_plan(int H0, int Ho, int Wo, int lds_budget, int* band_rows, int* tile_rows,
                              int* lds_bytes) {
  VS_CHECK_ARG(H0 > 0 && Ho > 0 && Wo > 0 && band_rows && tile_rows && lds_bytes, "bad args");
  const bool need_v = H0 != Ho;
  const int ksize_v = need_v ? vs_resize_ksize(H0, Ho) : 0;
  for (int band = Ho < IG_MAX_BAND ? Ho : IG_MAX_BAND; band >= 1; --band) {
    int rows = band;
    if (need_v) {
      rows = 0;
      for (int y0 = 0; y0 < Ho; y0 += band) {
        const int y1 = (y0 + band < Ho ? y0 + band : Ho) - 1;
        int lo, hi, cnt;
        ig_window(H0, Ho, y0, &lo, &cnt);
        ig_window(H0, Ho, y1, &hi, &cnt);
        if (hi + cnt - lo > rows) rows = hi + cnt - lo;
      }
    }
    const size_t need = ig_lds_bytes(band, rows, Wo, ksize_v);
    if (need <= (size_t)lds_budget) {
      *band_rows = band;
      *tile_rows = rows;
      *lds_bytes = (int)need;
      return VS_OK;
    }
  }
  vs_set_error("%s: one output row of %d x 3 bytes from %d source rows does not fit %d bytes of LDS", __func__, Wo,
               H0, lds_budget);
  return VS_ERR_BAD_ARG;
}

struct __attribute__((packed, aligned(1))) ig_taps4 {
  uint32_t a, b, c;  // 4 RGB taps
};

__device__ __forceinline__ uint32_t ig_clip8(int v) {
  v >>= IG_PRECISION_BITS;
  return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

__device__ __forceinline__ int ig_byte(uint32_t w, int k) { return (int)((w >> (8 * k)) & 0xffu); }

struct ig_args {
  const uint8_t* src;
  uint16_t* y_fast;
  uint16_t* y_slow;
  const int* t_slow;
  const int* bounds_h;
  const int* kk_h;
  const int* bounds_v;
  const int* kk_v;
  int T, Tslow, H0, W0, Ho, Wo, ksize_h, ksize_v, cpad_fast, cpad_slow, band, tile_rows, nbands, reverse;
  float m0, m1, m2, s0, s1, s2;
};

__device__ __forceinline__ void ig_store_px(uint16_t* y, long long px, int cpad, uint32_t c01, uint32_t c2) {
  if (cpad == 4)
    *(uint2*)(y + px * 4) = make_uint2(c01, c2);
  else
    *(uint4*)(y + px * 8) = make_uint4(c01, c2, 0u, 0u);
}

template <bool HPASS, bool VPASS>
__global__ __launch_bounds__(IG_THREADS) void ingest_u8_kernel(const ig_args a) {
  extern __shared__ __align__(16) uint8_t ig_smem[];
  uint16_t* lut = (uint16_t*)ig_smem;                       // [3][256] bf16 bits of the normalised value
  int* kv_s = (int*)(ig_smem + IG_LUT_BYTES);               // [band][ksize_v]
  int* bv_s = kv_s + a.band * a.ksize_v;                    // [band][2]: first tile row, count
  uint8_t* tile = (uint8_t*)(bv_s + a.band * 2);            // [tile_rows][pitch]
  const int tid = threadIdx.x;
  const long long f = blockIdx.x / a.nbands;                // frame n * T + t
  const int b = blockIdx.x - (int)(f * a.nbands);
  const int Wo = a.Wo, pitch = (Wo + 3) / 4 * 12;
  const int yo0 = b * a.band;
  const int nyo = min(a.band, a.Ho - yo0);

  // source rows of the band (block-uniform)
  int y_lo = yo0, rows = nyo;
  if (VPASS) {
    y_lo = max(a.bounds_v[yo0 * 2], 0);
    const int y_hi = min(a.bounds_v[(yo0 + nyo - 1) * 2] + a.bounds_v[(yo0 + nyo - 1) * 2 + 1], a.H0);
    rows = min(y_hi - y_lo, a.tile_rows);
  }

  // ---- tables: the normalisation of every byte value, the band's vertical weights
  {
    const float mean[3] = {a.m0, a.m1, a.m2}, sd[3] = {a.s0, a.s1, a.s2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float x = (float)tid / 255.0f;      // tensor.float() / 255.0
      lut[c * 256 + tid] = f32_to_bf16((x - mean[c]) / sd[c]);  // (tensor - mean) / std, one rounding
    }
    if (VPASS) {
      for (int i = tid; i < nyo * a.ksize_v; i += IG_THREADS) {
        const int r = i / a.ksize_v;
        kv_s[i] = a.kk_v[(long long)(yo0 + r) * a.ksize_v + (i - r * a.ksize_v)];
      }
      for (int r = tid; r < nyo; r += IG_THREADS) {
        int first = a.bounds_v[(yo0 + r) * 2] - y_lo, cnt = min(a.bounds_v[(yo0 + r) * 2 + 1], a.ksize_v);
        first = min(max(first, 0), rows);
        bv_s[r * 2] = first;
        bv_s[r * 2 + 1] = max(min(cnt, rows - first), 0);
      }
    }
  }

  // ---- 1. horizontal pass (or a copy) of source rows y_lo .. y_lo + rows into the tile
  const uint8_t* fsrc = a.src + (f * a.H0 + y_lo) * (long long)a.W0 * 3;
  if (HPASS) {
    const float rcp = 1.0f / (float)Wo;
    for (int i = tid; i < rows * Wo; i += IG_THREADS) {
      int r, xo;
      fast_divmod(i, Wo, rcp, r, xo);
      const int xmin = min(max(a.bounds_h[xo * 2], 0), a.W0);
      const int cnt = max(min(min(a.bounds_h[xo * 2 + 1], a.ksize_h), a.W0 - xmin), 0);
      const int* k = a.kk_h + (long long)xo * a.ksize_h;
      const uint8_t* p = fsrc + ((long long)r * a.W0 + xmin) * 3;
      int s0 = 1 << (IG_PRECISION_BITS - 1), s1 = s0, s2 = s0;
      int x = 0;
      for (; x + 4 <= cnt; x += 4) {
        ig_taps4 w;
        __builtin_memcpy(&w, p + x * 3, 12);
        const int k0 = k[x], k1 = k[x + 1], k2 = k[x + 2], k3 = k[x + 3];
        s0 += __mul24(ig_byte(w.a, 0), k0) + __mul24(ig_byte(w.a, 3), k1) + __mul24(ig_byte(w.b, 2), k2) +
              __mul24(ig_byte(w.c, 1), k3);
        s1 += __mul24(ig_byte(w.a, 1), k0) + __mul24(ig_byte(w.b, 0), k1) + __mul24(ig_byte(w.b, 3), k2) +
              __mul24(ig_byte(w.c, 2), k3);
        s2 += __mul24(ig_byte(w.a, 2), k0) + __mul24(ig_byte(w.b, 1), k1) + __mul24(ig_byte(w.c, 0), k2) +
              __mul24(ig_byte(w.c, 3), k3);
      }
      for (; x < cnt; ++x) {
        const int kx = k[x];
        s0 += __mul24((int)p[x * 3 + 0], kx);
        s1 += __mul24((int)p[x * 3 + 1], kx);
        s2 += __mul24((int)p[x * 3 + 2], kx);
      }
      uint8_t* o = tile + r * pitch + xo * 3;
      o[0] = (uint8_t)ig_clip8(s0);
      o[1] = (uint8_t)ig_clip8(s1);
      o[2] = (uint8_t)ig_clip8(s2);
    }
  } else {
    const int rb = Wo * 3;  // (W0 == Wo)
    const float rcp = 1.0f / (float)rb;
    for (int i = tid; i < rows * rb; i += IG_THREADS) {
      int r, xb;
      fast_divmod(i, rb, rcp, r, xb);
      tile[r * pitch + xb] = fsrc[(long long)r * rb + xb];
    }
  }
  __syncthreads();

  // ---- which slow-pathway slots take this frame (block-uniform)
  const long long n = f / a.T;
  const int t = (int)(f - n * a.T);
  int so_first = -1, so_more = 0;  // first slot that takes frame t; whether a later one does too (an index may repeat)
  for (int so = a.Tslow - 1; so >= 0; --so)
    if (a.t_slow[so] == t) {
      so_more = so_first >= 0;
      so_first = so;
    }

  // ---- 2. + 3. vertical pass of 4 pixels per thread, normalise, store
  const int W4 = (Wo + 3) / 4;
  const float rcp4 = 1.0f / (float)W4;
  const int r0 = a.reverse ? 2 : 0, r2 = a.reverse ? 0 : 2;
  for (int i = tid; i < nyo * W4; i += IG_THREADS) {
    int yl, j;
    fast_divmod(i, W4, rcp4, yl, j);
    uint32_t q[12];
    if (VPASS) {
      int s[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) s[e] = 1 << (IG_PRECISION_BITS - 1);
      const int first = bv_s[yl * 2], cnt = bv_s[yl * 2 + 1];
      const int* kv = kv_s + yl * a.ksize_v;
      const uint8_t* col = tile + first * pitch + j * 12;
      for (int y = 0; y < cnt; ++y) {
        const int ky = kv[y];
        const uint32_t* w = (const uint32_t*)(col + y * pitch);
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s[e] += __mul24(ig_byte(w0, e), ky);
          s[4 + e] += __mul24(ig_byte(w1, e), ky);
          s[8 + e] += __mul24(ig_byte(w2, e), ky);
        }
      }
#pragma unroll
      for (int e = 0; e < 12; ++e) q[e] = ig_clip8(s[e]);
    } else {
      const uint32_t* w = (const uint32_t*)(tile + yl * pitch + j * 12);
#pragma unroll
      for (int e = 0; e < 12; ++e) q[e] = (uint32_t)ig_byte(w[e >> 2], e & 3);
    }
    const int yo = yo0 + yl;
    const long long px_fast = (f * a.Ho + yo) * (long long)Wo + j * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (j * 4 + e >= Wo) break;
      const uint32_t c01 = (uint32_t)lut[q[e * 3 + r0]] | ((uint32_t)lut[256 + q[e * 3 + 1]] << 16);
      const uint32_t c2 = (uint32_t)lut[512 + q[e * 3 + r2]];
      ig_store_px(a.y_fast, px_fast + e, a.cpad_fast, c01, c2);
      if (so_first >= 0) {
        ig_store_px(a.y_slow, ((n * a.Tslow + so_first) * a.Ho + yo) * (long long)Wo + j * 4 + e, a.cpad_slow, c01,
                    c2);
        if (so_more)
          for (int so = so_first + 1; so < a.Tslow; ++so)
            if (a.t_slow[so] == t)
              ig_store_px(a.y_slow, ((n * a.Tslow + so) * a.Ho + yo) * (long long)Wo + j * 4 + e, a.cpad_slow, c01,
                          c2);
      }
    }
  }
}

extern "C" int vs_ingest_u8(const uint8_t* src, void* y_fast, void* y_slow, const int* t_index_slow, int N, int T,
                            int Tslow, int H0, int W0, int Ho, int Wo, const int32_t* bounds_h, const int32_t* kk_h,
                            int ksize_h, const int32_t* bounds_v, const int32_t* kk_v, int ksize_v, int cpad_fast,
                            int cpad_slow, const float* mean3, const float* std3, int reverse_channels,
                            void* stream) {
  VS_CHECK_ARG(src && y_fast && mean3 && std3, "null argument (mean3 / std3 are host pointers)");
  VS_CHECK_ARG(N > 0 && T > 0 && H0 > 0 && W0 > 0 && Ho > 0 && Wo > 0, "bad sizes");
  VS_CHECK_ARG(cpad_fast == 4 || cpad_fast == 8, "cpad_fast must be 4 or 8");
  VS_CHECK_ARG(Tslow >= 0 && (Tslow == 0 || (y_slow && t_index_slow && (cpad_slow == 4 || cpad_slow == 8))),
               "a slow pathway needs y_slow, t_index_slow and cpad_slow 4 or 8");
  const bool need_h = W0 != Wo, need_v = H0 != Ho;
  VS_CHECK_ARG(!need_h || (bounds_h && kk_h && ksize_h == vs_resize_ksize(W0, Wo)), "horizontal tables missing");
  VS_CHECK_ARG(!need_v || (bounds_v && kk_v && ksize_v == vs_resize_ksize(H0, Ho)), "vertical tables missing");
  VS_CHECK_ARG((long long)Ho * Wo < (1 << 24), "output frame too large");
  ig_args a;
  int lds = 0;
  int rc = vs_ingest_plan(H0, Ho, Wo, 64 * 1024, &a.band, &a.tile_rows, &lds);
  if (rc != VS_OK) return rc;
  a.nbands = (Ho + a.band - 1) / a.band;
  const long long blocks = (long long)N * T * a.nbands;
  VS_CHECK_ARG(blocks <= 0x7fffffffLL, "too many frames for one launch");
  a.src = src;
  a.y_fast = (uint16_t*)y_fast;
  a.y_slow = Tslow ? (uint16_t*)y_slow : nullptr;
  a.t_slow = t_index_slow;
  a.bounds_h = bounds_h;
  a.kk_h = kk_h;
  a.bounds_v = bounds_v;
  a.kk_v = kk_v;
  a.T = T, a.Tslow = Tslow, a.H0 = H0, a.W0 = W0, a.Ho = Ho, a.Wo = Wo;
  a.ksize_h = need_h ? ksize_h : 0, a.ksize_v = need_v ? ksize_v : 0;
  a.cpad_fast = cpad_fast, a.cpad_slow = cpad_slow, a.reverse = reverse_channels ? 1 : 0;
  a.m0 = mean3[0], a.m1 = mean3[1], a.m2 = mean3[2], a.s0 = std3[0], a.s1 = std3[1], a.s2 = std3[2];
  const dim3 grid((unsigned)blocks), block(IG_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (need_h && need_v)
    hipLaunchKernelGGL((ingest_u8_kernel<true, true>), grid, block, (size_t)lds, st, a);
  else if (need_h)
    hipLaunchKernelGGL((ingest_u8_kernel<true, false>), grid, block, (size_t)lds, st, a);
  else if (need_v)
    hipLaunchKernelGGL((ingest_u8_kernel<false, true>), grid, block, (size_t)lds, st, a);
  else
    hipLaunchKernelGGL((ingest_u8_kernel<false, false>), grid, block, (size_t)lds, st, a);
  VS_CHECK_LAUNCH();
  return VS_OK;
}
