// Sampling search (fairseq search.Sampling restated: plain, top-k, nucleus): one drawn token per row of a search step,
// and the step's bookkeeping with one candidate per beam.  docs/beam_search_parity.md, "Sampling", is the contract.
//
//   lp_j   the scoring rules of vs_beam_topk[_ngram] (beam_shared.h: bt_rule_lp), before the cumulative score
//   q_j    = rint(exp(lp_j - m) * 2^40), an INTEGER mass; m is the row's largest lp after the rules, so the likeliest
//          allowed token weighs 2^40 however unlikely it is (eos alone at max_len, a forced token) and the masses sum
//          below 2^64.  Every sum below is a sum of integers: it has no order, needs no floating-point atomics, and is
//          the same number in the one-block and the sliced form by construction.  The rounding is below 2^-41 of the
//          largest mass per token (2.3e-8 of it over 50 k tokens).
//   key_j  an order-preserving 32-bit image of lp_j; equal keys <=> equal lp <=> equal q
//   kept   the tokens ranked (key descending, token ascending) before a threshold: an MSB-first radix select over the
//          key's four bytes (256 bins of count and mass per pass) finds the key T at which the rank k (top-k) or the
//          cumulative mass t (nucleus: the token that crosses t is kept) falls; of the tokens with key == T the `need`
//          lowest ids are kept.  Plain sampling keeps everything (a token of mass 0 cannot be drawn).
//          The nucleus threshold is topp * exp(-m) * 2^40 in the same units (beyond 2^64: everything is kept).
//   draw   target = floor((w + 0.5) * 2^-32 * S), S the kept mass, w the Philox word of element `row id` at the
//          search's (seed, step) and site VS_SAMPLE_SITE; the token whose interval of the kept masses' running sum in
//          ascending token id holds `target`.  S = 0: (-inf, token 0).
//
// Two forms.  Sliced (a workspace, V > BT_SLICE): grid = slices x rows per pass, the bins of a row are added up in
// global memory with integer atomics, every launch resolves the previous pass's bins on its own (256 bins: one block
// scan).  One block per row (no workspace, or one slice): the same device functions over the slices in turn, bins and
// per-slice totals in LDS.
#include <math.h>

#include "beam_shared.h"
#include "common.h"
#include "dropout_rng.h"

#define SM_ONE 1099511627776.f      // 2^40
#define SM_MAX_SLICES_ONE_BLOCK 32  // one block per row: V <= 65536

struct SmSel {        // the selection of one row after a radix pass
  uint32_t prefix;    // the threshold key's bytes found so far (the whole key T after four passes)
  uint32_t all;       // 1: the threshold lies behind the last token, everything is kept (T = 0, need = 0)
  uint32_t krem;      // top-k: ranks still to fill at or below the prefix
  uint32_t need;      // after the last pass: how many tokens with key == T are kept, lowest ids first
  uint64_t trem;      // nucleus: mass still missing at or below the prefix
  uint64_t qT;        // after the last pass: the mass of one token with key == T
};

struct SampleP {
  const float* logits; const float* cum; const int64_t* forced; const int64_t* tokens;
  const int64_t* snap; const int64_t* row_ids;
  float* out_val; int64_t* out_idx;
  int tok_ld, step, ngram, V, S, pad, eos, unk, flags, mode, k;  // mode 0 plain, 1 top-k, 2 nucleus
  float unk_penalty, inv_temp;
  double topp;
  // sliced form (workspace)
  float2* part;        // [rows][S]
  float* lmax;         // [rows][S]  largest lp after the rules of a slice
  uint32_t* hcnt;      // [4][rows][256]
  uint64_t* hmass;     // [4][rows][256]
  SmSel* sel;          // [4][rows]
  uint32_t* tiecnt;    // [rows][S]  tokens with key == T of a slice
  uint64_t* above;     // [rows][S]  mass of the tokens with key > T of a slice
};

__device__ __forceinline__ uint32_t sm_key(float lp) {
  const uint32_t b = __float_as_uint(lp == 0.f ? 0.f : lp);  // -0 and +0 are one rank
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// lp, key and mass of this thread's BT_E tokens of slice sl (token sl * BT_SLICE + e * 256 + tid); tokens past V get
// key 0 (below every real key: a rule's -inf has key 0x007FFFFF) and mass 0.  BAN: bm is the slice's ban bitmap
// (BT_SLICE / 32 words of LDS), rebuilt here.
template <bool BAN>
__device__ __forceinline__ void sm_slice_vals(const SampleP& p, int r, int sl, const BtRules& R, float m, unsigned* bm,
                                              int tid, float* lp, uint32_t* key, uint64_t* q) {
  const float* x = p.logits + (long long)r * p.V;
  if (BAN) {
    __syncthreads();  // earlier readers of bm are done
    if (tid < BT_SLICE / 32) bm[tid] = 0u;
    __syncthreads();
    bt_mark_banned(p.tokens + (long long)r * p.tok_ld, p.step, p.ngram, sl * BT_SLICE, BT_SLICE, p.V, bm, tid);
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < BT_E; ++e) {
    const int j = sl * BT_SLICE + e * 256 + tid;
    const bool ok = j < p.V;
    const float v = bt_rule_lp(R, x[ok ? j : 0], j, BAN && ((bm[(e * 256 + tid) >> 5] >> (tid & 31)) & 1u));
    lp[e] = v;
    key[e] = ok ? sm_key(v) : 0u;
    q[e] = (ok && v != -INFINITY) ? (uint64_t)llrintf(expf(v - m) * SM_ONE) : 0ull;  // v <= m: at most 2^40
  }
}

// The largest lp after the rules of slice sl, to every thread.  red: 4 floats of LDS.  A maximum has no rounding.
template <bool BAN>
__device__ __forceinline__ float sm_slice_max(const SampleP& p, int r, int sl, const BtRules& R, unsigned* bm,
                                              float* red, int tid) {
  float lp[BT_E];
  uint32_t key[BT_E];
  uint64_t q[BT_E];
  sm_slice_vals<BAN>(p, r, sl, R, 0.f, bm, tid, lp, key, q);
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < BT_E; ++e)
    if (sl * BT_SLICE + e * 256 + tid < p.V) mx = fmaxf(mx, lp[e]);
  mx = wave_reduce_max(mx);
  __syncthreads();  // earlier readers of red are done
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// topp in the units of the row's masses; past 2^64 no sum reaches it: everything is kept.
__device__ __forceinline__ uint64_t sm_topp_units(double topp, float m) {
  const double t = topp * exp(-(double)m) * 1099511627776.0;
  return t >= 1.8e19 ? 0xFFFFFFFFFFFFFFFFull : (t < 1.0 ? 1ull : (uint64_t)rint(t));
}

// Inclusive scan of (c, m) over the 256 threads of the block in thread order.  wc / wm: 4 words of LDS each.
__device__ __forceinline__ void sm_block_scan(uint32_t& c, uint64_t& m, uint32_t* wc, uint64_t* wm, int tid) {
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t oc = __shfl_up(c, o, 64);
    const uint32_t lo = __shfl_up((uint32_t)m, o, 64), hi = __shfl_up((uint32_t)(m >> 32), o, 64);
    if (lane >= o) {
      c += oc;
      m += ((uint64_t)hi << 32) | lo;
    }
  }
  __syncthreads();  // earlier readers of wc / wm are done
  if (lane == 63) {
    wc[w] = c;
    wm[w] = m;
  }
  __syncthreads();
  for (int i = 0; i < w; ++i) {
    c += wc[i];
    m += wm[i];
  }
}

// Adds this thread's tokens that match the prefix above byte d (d = 0: all) to the bins of byte d.
__device__ __forceinline__ void sm_hist_add(const uint32_t* key, const uint64_t* q, const SmSel& s, int d,
                                            uint32_t* hc, uint64_t* hm, int V, int sl, int tid) {
  const int shift = 24 - 8 * d;
#pragma unroll
  for (int e = 0; e < BT_E; ++e) {
    const bool ok = sl * BT_SLICE + e * 256 + tid < V;
    const bool match = d == 0 || (key[e] >> (shift + 8)) == (s.prefix >> (shift + 8));
    if (ok && match) {
      const int b = (key[e] >> shift) & 255;
      atomicAdd(&hc[b], 1u);
      if (q[e]) atomicAdd((unsigned long long*)&hm[b], (unsigned long long)q[e]);
    }
  }
}

// Pass d's bins (count hc, mass hm: 256 each, LDS or global) -> the selection after pass d in *out (LDS), from the
// selection `in` before it.  Thread tid owns bin 255 - tid, so thread order is key-descending; the bin in which the
// rank / the mass crosses is unique and not empty.  Ends with a __syncthreads: *out is readable by the block.
__device__ __forceinline__ void sm_resolve(const uint32_t* hc, const uint64_t* hm, const SmSel in, SmSel* out, int d,
                                           int mode, uint32_t* wc, uint64_t* wm, int tid) {
  const int b = 255 - tid, shift = 24 - 8 * d;
  const uint32_t c0 = hc[b];
  const uint64_t m0 = hm[b];
  uint32_t c = c0;
  uint64_t m = m0;
  if (tid == 0) {  // nobody crosses: everything is kept
    SmSel s = in;
    s.all = 1; s.prefix = 0; s.need = 0; s.qT = 0;
    *out = s;
  }
  sm_block_scan(c, m, wc, wm, tid);  // its syncs order the default above before the store below
  const uint32_t ec = c - c0;
  const uint64_t em = m - m0;
  const bool cross = !in.all && (mode == 1 ? (ec < in.krem && in.krem <= c) : (em < in.trem && in.trem <= m));
  if (cross) {
    SmSel s;
    s.prefix = in.prefix | ((uint32_t)b << shift);
    s.all = 0;
    s.krem = in.krem - ec;
    s.trem = in.trem - em;
    s.qT = c0 ? m0 / c0 : 0;  // the last pass's bin holds one key: equal masses
    s.need = mode == 1 ? s.krem : (uint32_t)((s.trem + s.qT - 1) / (s.qT ? s.qT : 1));
    *out = s;
  }
  __syncthreads();
}

// Tokens with key == T and the mass above T of this thread's tokens, added to two LDS words.
__device__ __forceinline__ void sm_tie_add(const uint32_t* key, const uint64_t* q, uint32_t T, uint32_t* tc,
                                           uint64_t* ab) {
  uint32_t c = 0;
  uint64_t m = 0;
#pragma unroll
  for (int e = 0; e < BT_E; ++e) {
    c += key[e] == T ? 1u : 0u;  // a token past V has key 0; T = 0 only with need = 0
    m += key[e] > T ? q[e] : 0ull;
  }
  if (c) atomicAdd(tc, c);
  if (m) atomicAdd((unsigned long long*)ab, (unsigned long long)m);
}

struct SmDraw {  // what thread 0 finds from the slices' totals
  uint64_t S, rel;   // kept mass of the row; target minus the kept mass of the slices before `slice`
  uint32_t tb;       // tokens with key == T in the slices before `slice`
  int slice;
  int found, last;   // the scan of the slice: a thread's interval held the target; the slice's last kept token
};

// The draw of row r: tc / ab are the row's per-slice totals (LDS or global), sel its final selection, dr / wc / wm /
// found LDS.  BAN as in sm_slice_vals.  Writes out_val[r], out_idx[r].
template <bool BAN>
__device__ __forceinline__ void sm_draw(const SampleP& p, int r, const BtRules& R, float m, const SmSel sel, const uint32_t* tc,
                                        const uint64_t* ab, SmDraw* dr, unsigned* bm, uint32_t* wc, uint64_t* wm,
                                        int tid) {
  if (tid == 0) {
    uint64_t S = 0;
    uint32_t tb = 0;
    for (int sl = 0; sl < p.S; ++sl) {
      const uint32_t kt = tb >= sel.need ? 0u : min(sel.need - tb, tc[sl]);
      S += ab[sl] + (uint64_t)kt * sel.qT;
      tb += tc[sl];
    }
    const uint64_t e = p.row_ids ? (uint64_t)p.row_ids[r] : (uint64_t)r;
    const vs_philox_out o = vs_dropout_block((uint64_t)p.snap[0], (uint64_t)p.snap[1], VS_SAMPLE_SITE, e >> 2);
    const uint64_t w2 = 2ull * o.w[e & 3] + 1ull;  // (w + 0.5) * 2^-32 = w2 * 2^-33
    const uint64_t target = (__umul64hi(w2, S) << 31) | ((w2 * S) >> 33);  // floor(w2 * S / 2^33) < S
    SmDraw d;
    d.S = S; d.slice = 0; d.rel = 0; d.tb = 0; d.found = 0; d.last = -1;
    uint64_t acc = 0;
    tb = 0;
    for (int sl = 0; sl < p.S; ++sl) {
      const uint32_t kt = tb >= sel.need ? 0u : min(sel.need - tb, tc[sl]);
      const uint64_t m = ab[sl] + (uint64_t)kt * sel.qT;
      if (target < acc + m) {
        d.slice = sl; d.rel = target - acc; d.tb = tb;
        break;
      }
      acc += m;
      tb += tc[sl];
    }
    *dr = d;
  }
  __syncthreads();
  const SmDraw d = *dr;
  if (d.S == 0) {  // nothing can be drawn: a live -inf candidate, as the beam search carries them
    if (tid == 0) {
      p.out_val[r] = -INFINITY;
      p.out_idx[r] = 0;
    }
    return;
  }
  float lp[BT_E];
  uint32_t key[BT_E];
  uint64_t q[BT_E];
  sm_slice_vals<BAN>(p, r, d.slice, R, m, bm, tid, lp, key, q);
  uint64_t acc = 0;     // kept mass of the slice's tokens before element group e
  uint32_t tb = d.tb;   // ties before element group e
  int last = -1;        // this thread's last kept token of positive mass, and its lp
  float last_lp = -INFINITY;
  for (int e = 0; e < BT_E; ++e) {  // ascending token id: groups of 256 consecutive tokens, thread order inside
    const uint32_t tie = key[e] == sel.prefix ? 1u : 0u;
    uint64_t m = key[e] > sel.prefix ? q[e] : 0ull;
    uint32_t cs = tie;  // ranks of the ties first: whether a tie is kept depends on its rank
    uint64_t z = 0;
    sm_block_scan(cs, z, wc, wm, tid);
    if (tie && tb + (cs - 1) < sel.need) m = q[e];
    const uint64_t m0 = m;
    uint32_t cz = 0;
    sm_block_scan(cz, m, wc, wm, tid);
    const uint64_t lo = acc + m - m0, hi = acc + m;
    if (m0) {
      last = d.slice * BT_SLICE + e * 256 + tid;
      last_lp = lp[e];
    }
    if (m0 && lo <= d.rel && d.rel < hi) {
      p.out_val[r] = lp[e] + (p.cum ? p.cum[r] : 0.f);
      p.out_idx[r] = d.slice * BT_SLICE + e * 256 + tid;
      dr->found = 1;
    }
    // totals of the group to every thread: the last thread's inclusive values
    __syncthreads();
    if (tid == 255) {
      wc[0] = cs;
      wm[0] = m;
    }
    __syncthreads();
    tb += wc[0];
    acc += wm[0];
  }
  // No interval held the target: the launches disagree on some token's mass (they recompute lp; it cannot happen
  // while they round alike).  The output is then the slice's last kept token, never unwritten memory.
  if (last >= 0) atomicMax(&dr->last, last);
  __syncthreads();
  if (!dr->found) {
    if (dr->last < 0) {
      if (tid == 0) {
        p.out_val[r] = -INFINITY;
        p.out_idx[r] = 0;
      }
    } else if (dr->last == last) {
      p.out_val[r] = last_lp + (p.cum ? p.cum[r] : 0.f);
      p.out_idx[r] = last;
    }
  }
}

// ---- sliced form ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sm_row_max(const float* lmax, int S) {
  float m = -INFINITY;
  for (int q = 0; q < S; ++q) m = fmaxf(m, lmax[q]);
  return m;
}

template <bool BAN>
__global__ __launch_bounds__(256) void sample_max_kernel(SampleP p) {
  __shared__ float red[4];
  __shared__ unsigned bm[BAN ? BT_SLICE / 32 : 1];
  const int sl = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const float lse = bt_lse_combine(p.part + (long long)r * p.S, p.S);
  const BtRules R = bt_rules(p.forced, r, p.pad, p.eos, p.unk, p.unk_penalty, p.inv_temp, p.flags, lse);
  const float mx = sm_slice_max<BAN>(p, r, sl, R, bm, red, tid);
  if (tid == 0) p.lmax[(size_t)r * p.S + sl] = mx;
  // the row's bins of the four radix passes start at zero: cleared here, by the launch before the first pass, not by
  // a memset -- a memset issued while the stream is capturing ran at capture time and not in the replays
  if (p.mode != 0 && sl == 0) {
    const size_t rows = gridDim.y;
    for (int i = tid; i < 4 * 256; i += 256) {
      const size_t o = ((size_t)(i >> 8) * rows + r) * 256 + (i & 255);
      p.hcnt[o] = 0u;
      p.hmass[o] = 0ull;
    }
  }
}

// Pass d of the radix select (d = 0..3), grid (S, rows): resolves pass d - 1 from the row's global bins, adds the
// slice's matching tokens to LDS bins and those to the row's global bins of pass d.
template <bool BAN>
__global__ __launch_bounds__(256) void sample_hist_kernel(SampleP p, int d) {
  __shared__ uint32_t hc[256];
  __shared__ uint64_t hm[256];
  __shared__ uint32_t wc[4];
  __shared__ uint64_t wm[4];
  __shared__ SmSel sel;
  __shared__ unsigned bm[BAN ? BT_SLICE / 32 : 1];
  const int sl = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, rows = gridDim.y;
  const float lse = bt_lse_combine(p.part + (long long)r * p.S, p.S);
  const BtRules R = bt_rules(p.forced, r, p.pad, p.eos, p.unk, p.unk_penalty, p.inv_temp, p.flags, lse);
  const float m = sm_row_max(p.lmax + (size_t)r * p.S, p.S);
  SmSel in;
  in.prefix = 0; in.all = 0; in.krem = (uint32_t)p.k; in.need = 0; in.qT = 0;
  in.trem = p.mode == 2 ? sm_topp_units(p.topp, m) : 0ull;
  hc[tid] = 0u;
  hm[tid] = 0ull;
  if (d > 0) {
    if (d > 1) in = p.sel[(size_t)(d - 2) * rows + r];
    sm_resolve(p.hcnt + ((size_t)(d - 1) * rows + r) * 256, p.hmass + ((size_t)(d - 1) * rows + r) * 256, in, &sel,
               d - 1, p.mode, wc, wm, tid);
    in = sel;
    if (sl == 0 && tid == 0) p.sel[(size_t)(d - 1) * rows + r] = in;
  }
  float lp[BT_E];
  uint32_t key[BT_E];
  uint64_t q[BT_E];
  sm_slice_vals<BAN>(p, r, sl, R, m, bm, tid, lp, key, q);
  __syncthreads();  // the zeroed bins
  if (!in.all) sm_hist_add(key, q, in, d, hc, hm, p.V, sl, tid);
  __syncthreads();
  if (hc[tid]) {
    atomicAdd(&p.hcnt[((size_t)d * rows + r) * 256 + tid], hc[tid]);
    if (hm[tid]) atomicAdd((unsigned long long*)&p.hmass[((size_t)d * rows + r) * 256 + tid], (unsigned long long)hm[tid]);
  }
}

// After the passes, grid (S, rows): resolves the last pass (top-k / nucleus), then the slice's tie count and mass
// above T.  Block 0 of a row stores the row's final selection for the draw.
template <bool BAN>
__global__ __launch_bounds__(256) void sample_tie_kernel(SampleP p) {
  __shared__ uint32_t wc[4];
  __shared__ uint64_t wm[4];
  __shared__ SmSel sel;
  __shared__ uint32_t tc;
  __shared__ uint64_t ab;
  __shared__ unsigned bm[BAN ? BT_SLICE / 32 : 1];
  const int sl = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, rows = gridDim.y;
  SmSel fin;
  fin.prefix = 0; fin.all = 1; fin.krem = 0; fin.need = 0; fin.trem = 0; fin.qT = 0;
  if (p.mode != 0) {
    sm_resolve(p.hcnt + ((size_t)3 * rows + r) * 256, p.hmass + ((size_t)3 * rows + r) * 256,
               p.sel[(size_t)2 * rows + r], &sel, 3, p.mode, wc, wm, tid);
    fin = sel;
  }
  if (tid == 0) {
    tc = 0u;
    ab = 0ull;
    if (sl == 0) p.sel[(size_t)3 * rows + r] = fin;
  }
  const float lse = bt_lse_combine(p.part + (long long)r * p.S, p.S);
  const BtRules R = bt_rules(p.forced, r, p.pad, p.eos, p.unk, p.unk_penalty, p.inv_temp, p.flags, lse);
  float lp[BT_E];
  uint32_t key[BT_E];
  uint64_t q[BT_E];
  sm_slice_vals<BAN>(p, r, sl, R, sm_row_max(p.lmax + (size_t)r * p.S, p.S), bm, tid, lp, key, q);
  __syncthreads();
  sm_tie_add(key, q, fin.prefix, &tc, &ab);
  __syncthreads();
  if (tid == 0) {
    p.tiecnt[(size_t)r * p.S + sl] = tc;
    p.above[(size_t)r * p.S + sl] = ab;
  }
}

template <bool BAN>
__global__ __launch_bounds__(256) void sample_draw_kernel(SampleP p) {
  __shared__ uint32_t wc[4];
  __shared__ uint64_t wm[4];
  __shared__ SmDraw dr;
  __shared__ unsigned bm[BAN ? BT_SLICE / 32 : 1];
  const int r = blockIdx.x, tid = threadIdx.x, rows = gridDim.x;
  const float lse = bt_lse_combine(p.part + (long long)r * p.S, p.S);
  const BtRules R = bt_rules(p.forced, r, p.pad, p.eos, p.unk, p.unk_penalty, p.inv_temp, p.flags, lse);
  sm_draw<BAN>(p, r, R, sm_row_max(p.lmax + (size_t)r * p.S, p.S), p.sel[(size_t)3 * rows + r],
               p.tiecnt + (size_t)r * p.S, p.above + (size_t)r * p.S, &dr, bm, wc, wm, tid);
}

// ---- one block per row: the same steps over the slices in turn, everything between them in LDS ------------------
template <bool BAN>
__global__ __launch_bounds__(256) void sample_row_kernel(SampleP p) {
  __shared__ float red[4];
  __shared__ float2 part[SM_MAX_SLICES_ONE_BLOCK];
  __shared__ uint32_t hc[256];
  __shared__ uint64_t hm[256];
  __shared__ uint32_t wc[4];
  __shared__ uint64_t wm[4];
  __shared__ SmSel sel;
  __shared__ uint32_t tc[SM_MAX_SLICES_ONE_BLOCK];
  __shared__ uint64_t ab[SM_MAX_SLICES_ONE_BLOCK];
  __shared__ SmDraw dr;
  __shared__ unsigned bm[BAN ? BT_SLICE / 32 : 1];
  const int r = blockIdx.x, tid = threadIdx.x;
  for (int sl = 0; sl < p.S; ++sl) {
    const float2 ms = bt_lse_slice(p.logits + (long long)r * p.V, sl, p.V, p.inv_temp, red, tid);
    if (tid == 0) part[sl] = ms;
  }
  __syncthreads();
  const float lse = bt_lse_combine(part, p.S);
  const BtRules R = bt_rules(p.forced, r, p.pad, p.eos, p.unk, p.unk_penalty, p.inv_temp, p.flags, lse);
  float lp[BT_E];
  uint32_t key[BT_E];
  uint64_t q[BT_E];
  float m = -INFINITY;
  for (int sl = 0; sl < p.S; ++sl) m = fmaxf(m, sm_slice_max<BAN>(p, r, sl, R, bm, red, tid));
  SmSel cur;
  cur.prefix = 0; cur.all = p.mode == 0; cur.krem = (uint32_t)p.k; cur.need = 0; cur.qT = 0;
  cur.trem = p.mode == 2 ? sm_topp_units(p.topp, m) : 0ull;
  if (p.mode != 0) {
    for (int d = 0; d < 4; ++d) {
      __syncthreads();
      hc[tid] = 0u;
      hm[tid] = 0ull;
      __syncthreads();
      if (!cur.all)
        for (int sl = 0; sl < p.S; ++sl) {
          sm_slice_vals<BAN>(p, r, sl, R, m, bm, tid, lp, key, q);
          sm_hist_add(key, q, cur, d, hc, hm, p.V, sl, tid);
        }
      __syncthreads();
      sm_resolve(hc, hm, cur, &sel, d, p.mode, wc, wm, tid);
      cur = sel;
    }
  }
  if (tid < SM_MAX_SLICES_ONE_BLOCK) {
    tc[tid] = 0u;
    ab[tid] = 0ull;
  }
  __syncthreads();
  for (int sl = 0; sl < p.S; ++sl) {
    sm_slice_vals<BAN>(p, r, sl, R, m, bm, tid, lp, key, q);
    sm_tie_add(key, q, cur.prefix, &tc[sl], &ab[sl]);
  }
  __syncthreads();
  sm_draw<BAN>(p, r, R, m, cur, tc, ab, &dr, bm, wc, wm, tid);
}

static inline size_t sm_align(size_t n) { return (n + 255) & ~(size_t)255; }

extern "C" size_t vs_sample_token_workspace_bytes(int rows, int V) {
  const size_t R = (size_t)rows, S = (size_t)bt_slices(V);
  return sm_align(R * S * 8) + sm_align(R * S * 4) + sm_align(4 * R * 256 * 4) + sm_align(4 * R * 256 * 8) + sm_align(4 * R * sizeof(SmSel)) +
         sm_align(R * S * 4) + sm_align(R * S * 8);
}

template <bool BAN>
static void sm_launch(SampleP p, int rows, bool sliced, void* workspace, hipStream_t stream) {
  if (!sliced) {
    hipLaunchKernelGGL(sample_row_kernel<BAN>, dim3(rows), dim3(256), 0, stream, p);
    return;
  }
  const size_t R = (size_t)rows, S = (size_t)p.S;
  char* w = (char*)workspace;
  p.part = (float2*)w;      w += sm_align(R * S * 8);
  p.lmax = (float*)w;       w += sm_align(R * S * 4);
  p.hcnt = (uint32_t*)w;    w += sm_align(4 * R * 256 * 4);
  p.hmass = (uint64_t*)w;   w += sm_align(4 * R * 256 * 8);
  p.sel = (SmSel*)w;        w += sm_align(4 * R * sizeof(SmSel));
  p.tiecnt = (uint32_t*)w;  w += sm_align(R * S * 4);
  p.above = (uint64_t*)w;
  hipLaunchKernelGGL(beam_lse_part_kernel, dim3(p.S, rows), dim3(256), 0, stream, p.logits, p.part, p.V, p.inv_temp);
  hipLaunchKernelGGL(sample_max_kernel<BAN>, dim3(p.S, rows), dim3(256), 0, stream, p);
  if (p.mode != 0) {
    for (int d = 0; d < 4; ++d)
      hipLaunchKernelGGL(sample_hist_kernel<BAN>, dim3(p.S, rows), dim3(256), 0, stream, p, d);
  }
  hipLaunchKernelGGL(sample_tie_kernel<BAN>, dim3(p.S, rows), dim3(256), 0, stream, p);
  hipLaunchKernelGGL(sample_draw_kernel<BAN>, dim3(rows), dim3(256), 0, stream, p);
}

extern "C" int vs_sample_token(const float* logits, const float* cum, const int64_t* forced, const int64_t* tokens,
                               int tok_ld, int step, int ngram, const int64_t* snap, const int64_t* row_ids,
                               float* out_val, int64_t* out_idx, int rows, int V, int topk, double topp, int pad,
                               int eos, int unk, float unk_penalty, float temperature, int flags, void* workspace,
                               size_t ws_bytes, void* stream) {
  VS_CHECK_ARG(logits && snap && out_val && out_idx && rows > 0 && V > 1, "bad args");
  VS_CHECK_ARG(temperature > 0.f, "temperature must be > 0");
  VS_CHECK_ARG(!(topk > 0 && topp > 0.0), "sampling_topk and sampling_topp exclude each other");
  VS_CHECK_ARG(topp <= 1.0, "sampling_topp must lie in (0, 1]");
  VS_CHECK_ARG(ngram >= 0 && ngram != 1, "ngram must be 0 or >= 2");
  VS_CHECK_ARG(ngram == 0 || (tokens && step >= 0 && step < tok_ld), "ngram > 0 needs the token history, step in [0, tok_ld)");
  const int S = bt_slices(V);
  const bool sliced = workspace && S >= 2;
  VS_CHECK_ARG(sliced || S <= SM_MAX_SLICES_ONE_BLOCK, "one block per row holds at most 65536 tokens: pass a workspace");
  VS_CHECK_ARG(!sliced || ws_bytes >= vs_sample_token_workspace_bytes(rows, V), "workspace too small");
  SampleP p = {};
  p.logits = logits; p.cum = cum; p.forced = forced; p.tokens = tokens; p.snap = snap; p.row_ids = row_ids;
  p.out_val = out_val; p.out_idx = out_idx;
  p.tok_ld = tok_ld; p.step = step; p.ngram = ngram; p.V = V; p.S = S; p.pad = pad; p.eos = eos; p.unk = unk;
  p.flags = flags; p.unk_penalty = unk_penalty; p.inv_temp = 1.0f / temperature;
  p.mode = topk > 0 ? 1 : topp > 0.0 ? 2 : 0;
  p.k = topk > V ? V : topk;
  p.topp = topp;
  if (ngram > 0)
    sm_launch<true>(p, rows, sliced, workspace, (hipStream_t)stream);
  else
    sm_launch<false>(p, rows, sliced, workspace, (hipStream_t)stream);
  VS_CHECK_LAUNCH();
  return VS_OK;
}

// ---- the step's bookkeeping with one candidate per beam (rule 5): candidate c of a sentence is (parent beam c, row
// c's draw); no merge, no sorting.  From "finalize" on it is vs_beam_step's code (bs_finish_step) with ncand = beam.
__global__ __launch_bounds__(64) void sample_step_kernel(BeamStepP p) {
  __shared__ float cv[BS_MAXC];
  __shared__ int ct[BS_MAXC];
  __shared__ int cb[BS_MAXC];
  __shared__ int act[BS_MAXC];
  __shared__ int sh_new_fin;
  const int s = blockIdx.x, lane = threadIdx.x;
  const long long row0 = (long long)s * p.beam;
  if (p.finished[s]) {
    bs_idle_rows(p, row0, lane);
    return;
  }
  if (lane < p.beam) {
    cv[lane] = p.row_val[row0 + lane];
    ct[lane] = (int)p.row_idx[row0 + lane];
    cb[lane] = lane;
  }
  __syncthreads();
  bs_finish_step(p, s, lane, p.beam, cv, ct, cb, act, &sh_new_fin);
}

extern "C" int vs_sample_step(const float* row_val, const int64_t* row_idx, const int64_t* tok_in, int64_t* tok_out,
                              const float* sc_in, float* sc_out, uint8_t* ignore, uint8_t* finished, int* nfin,
                              int* remaining, int64_t* fin_tok, float* fin_score, float* fin_pos, int* fin_len,
                              int64_t* reorder, const int32_t* anc_in, int32_t* anc_out, int anc_ld, int bsz, int beam,
                              int step, int max_len, int eos, int normalize, float len_penalty, void* stream) {
  VS_CHECK_ARG(row_val && row_idx && tok_in && tok_out && sc_in && sc_out && ignore && finished && nfin &&
                   remaining && fin_tok && fin_score && fin_pos && fin_len && reorder, "null argument");
  VS_CHECK_ARG(bsz > 0 && beam >= 1 && beam <= BS_MAXC, "beam <= 64");
  VS_CHECK_ARG(step >= 0 && step <= max_len, "step must be in [0, max_len]");
  VS_CHECK_ARG((anc_in == nullptr) == (anc_out == nullptr) && (!anc_out || anc_ld > step), "ancestry tables");
  const BeamStepP p = bs_params(row_val, row_idx, tok_in, tok_out, sc_in, sc_out, ignore, finished, nfin, remaining,
                                fin_tok, fin_score, fin_pos, fin_len, reorder, anc_in, anc_out, anc_ld, beam, 1, 0,
                                step, max_len, eos, normalize, len_penalty);
  hipLaunchKernelGGL(sample_step_kernel, dim3(bsz), dim3(64), 0, (hipStream_t)stream, p);
  VS_CHECK_LAUNCH();
  return VS_OK;
}
