// What the beam-search kernels (gpt2_ops.hip) and the sampling kernels (sample_ops.hip) share: the scoring rules of one
// search step, the n-gram ban bitmap, the per-slice log-sum-exp partials, and the bookkeeping of a step from
// "finalize" on.  Each exists once, here; the callers differ in what they do with the scored row (k best entries /
// a drawn token) and in how a sentence's candidates are formed (cross-beam merge / one draw per beam).
#pragma once
#include <math.h>

#include "common.h"

// ---- large vocabularies: the row is cut into slices of BT_SLICE tokens, element e * 256 + tid of a slice per thread
#define BT_SLICE 2048
#define BT_E (BT_SLICE / 256)

static inline int bt_slices(int V) { return (V + BT_SLICE - 1) / BT_SLICE; }
static inline size_t bt_bitmap_bytes(int V) { return (((size_t)V + 31) / 32) * 4; }  // one-block ban bitmap

// Sets bit t - base of bm for every banned token t in [base, base + nbits) of one row: threads stride
// over the start positions i of the earlier n-1-grams, n-1 compares each against the suffix
// row[step+2-n .. step]; the follower row[i+n-1] lies at or before `step` -- nothing after it is read
// (the tail of the search's token buffer is uninitialised).  step + 2 - n < 0: no start position,
// nothing banned (:756).  The caller zeroes bm and syncs before, and syncs after; a set has no order.
__device__ __forceinline__ void bt_mark_banned(const int64_t* row, int step, int n, int base, int nbits,
                                               int V, unsigned* bm, int tid) {
  const int s0 = step + 2 - n;
  for (int i = tid; i < s0; i += 256) {
    bool eq = true;
    for (int j = 0; j < n - 1 && eq; ++j) eq = row[i + j] == row[s0 + j];
    if (!eq) continue;
    const long long t = row[i + n - 1];
    if (t < base || t >= V || t - base >= nbits) continue;
    const int o = (int)(t - base);
    atomicOr(&bm[o >> 5], 1u << (o & 31));
  }
}

// The rules of one row at one step (seq_gen.py:318-353): everything that is the same for every token of the row.
struct BtRules {
  int pad, eos, unk, flags;  // flags & 1: only eos allowed (step >= max_len); & 2: eos banned (step < min_len)
  float unk_penalty, inv_temp, lse;
  long long f;  // forced token of the row (prefix forcing), < 0 or == pad: none
  bool force;
};

__device__ __forceinline__ BtRules bt_rules(const int64_t* forced, int r, int pad, int eos, int unk,
                                            float unk_penalty, float inv_temp, int flags, float lse) {
  BtRules R;
  R.pad = pad; R.eos = eos; R.unk = unk; R.flags = flags;
  R.unk_penalty = unk_penalty; R.inv_temp = inv_temp; R.lse = lse;
  R.f = forced ? forced[r] : -1;
  R.force = R.f >= 0 && R.f != pad;
  return R;
}

// lp of token j with logit xj: log-softmax at the temperature, NaN -> -inf, pad, unk penalty, eos-only, prefix
// forcing / eos ban, n-gram ban (`banned`).  The one statement of the rule list; the cumulative score is the caller's.
__device__ __forceinline__ float bt_rule_lp(const BtRules& R, float xj, int j, bool banned) {
  // spelled out: the sampling kernels recompute lp in seven launches and rank by its bits, so which product fuses
  // is not left to each inlining context (the compiler fused it in the beam kernels already: their bits stay)
  float lp = __fmaf_rn(xj, R.inv_temp, -R.lse);
  if (lp != lp) lp = -INFINITY;
  if (j == R.pad) lp = -INFINITY;
  if (j == R.unk) lp -= R.unk_penalty;
  if ((R.flags & 1) && j != R.eos) lp = -INFINITY;
  if (R.force) {
    if (j != (int)R.f) lp = -INFINITY;
  } else if ((R.flags & 2) && j == R.eos) {
    lp = -INFINITY;
  }
  if (banned) lp = -INFINITY;
  return lp;
}

// (max, sum exp(. - max)) of slice sl of a row at the temperature, by a block of 256 threads; every thread returns the
// pair.  red: 4 floats of LDS.  Fixed order: 8 elements per thread, wave butterfly, four waves.
__device__ __forceinline__ float2 bt_lse_slice(const float* x, int sl, int V, float inv_temp, float* red, int tid) {
  float v[BT_E];
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < BT_E; ++e) {
    const int j = sl * BT_SLICE + e * 256 + tid;
    const bool ok = j < V;
    const float t = x[ok ? j : 0] * inv_temp;
    v[e] = ok ? t : -INFINITY;
    mx = fmaxf(mx, v[e]);
  }
  mx = wave_reduce_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
#pragma unroll
  for (int e = 0; e < BT_E; ++e) {
    const int j = sl * BT_SLICE + e * 256 + tid;
    // a -inf logit adds exactly 0; written out so that a slice of nothing but -inf (mx = -inf) gives 0 and
    // not exp(-inf - -inf) = NaN, which would turn the whole row into -inf (a NaN logit still does)
    if (j < V) sum += v[e] == -INFINITY ? 0.f : expf(v[e] - mx);
  }
  sum = wave_reduce_sum(sum);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  const float2 out = make_float2(mx, (red[0] + red[1]) + (red[2] + red[3]));
  __syncthreads();  // red may be reused at once
  return out;
}

// grid (slices, rows): part[r][sl] = bt_lse_slice.  One source for both translation units that launch it.
static __global__ __launch_bounds__(256) void beam_lse_part_kernel(const float* logits, float2* part, int V,
                                                                   float inv_temp) {
  __shared__ float red[4];
  const int sl = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, S = gridDim.x;
  const float2 ms = bt_lse_slice(logits + (long long)r * V, sl, V, inv_temp, red, tid);
  if (tid == 0) part[(long long)r * S + sl] = ms;
}

// The row's log-sum-exp from its S slice partials, in slice order: the same bits in every block that asks.
__device__ __forceinline__ float bt_lse_combine(const float2* part, int S) {
  float M = -INFINITY;
  for (int q = 0; q < S; ++q) M = fmaxf(M, part[q].x);
  float sum = 0.f;
  for (int q = 0; q < S; ++q) {
    const float2 pq = part[q];
    sum += pq.y * expf(pq.x - M);
  }
  return M + logf(sum);
}

// =============================================================================================
// Device-side search bookkeeping of one step, one block of 64 threads per sentence.
// =============================================================================================
struct BeamStepP {
  const float* row_val;     // [bsz*beam][k]   per-row top-k of vs_beam_topk (cumulative scores added)
  const int64_t* row_idx;   // [bsz*beam][k]
  const int64_t* tok_in;    // [bsz*beam][Lt]  Lt = max_len + 2
  int64_t* tok_out;
  const float* sc_in;       // [bsz*beam][Ls]  Ls = max_len + 1
  float* sc_out;
  uint8_t* ignore;          // [bsz][beam]     cands_to_ignore
  uint8_t* finished;        // [bsz]
  int* nfin;                // [bsz]           hypotheses finalized so far
  int* remaining;           // [1]             sentences not finished yet
  int64_t* fin_tok;         // [bsz][beam][Ls] finalized token sequences (eos included)
  float* fin_score;         // [bsz][beam]
  float* fin_pos;           // [bsz][beam][Ls] positional scores
  int* fin_len;             // [bsz][beam]
  int64_t* reorder;         // [bsz*beam]      parent row of every new row (KV-cache gather index)
  const int* anc_in;        // [bsz*beam][anc_ld] or NULL: cache row holding position j of the hypothesis
  int* anc_out;             //                  (vs_attn_decode's ancestry table; replaces the gather)
  int anc_ld;
  int beam, k, V, step, max_len, Lt, Ls, eos, normalize;
  float len_penalty;
};

#define BS_MAXC 64  // 2 * beam candidates kept per sentence (beam <= 32)

__device__ __forceinline__ void bs_anc_row(const BeamStepP& p, long long nrow, long long prow, int lane) {
  if (!p.anc_out) return;
  for (int j = lane; j <= p.step + 1 && j < p.anc_ld; j += 64)
    p.anc_out[nrow * p.anc_ld + j] = j <= p.step ? p.anc_in[prow * p.anc_ld + j] : (int)nrow;
}

// A sentence that is (or has just become) finished: its rows carry their state over unchanged.
__device__ __forceinline__ void bs_idle_rows(const BeamStepP& p, long long row0, int lane) {
  for (int b = 0; b < p.beam; ++b) {
    for (int j = lane; j < p.Lt; j += 64) p.tok_out[(row0 + b) * p.Lt + j] = p.tok_in[(row0 + b) * p.Lt + j];
    for (int j = lane; j < p.Ls; j += 64) p.sc_out[(row0 + b) * p.Ls + j] = p.sc_in[(row0 + b) * p.Ls + j];
    if (lane == 0) p.reorder[row0 + b] = row0 + b;
    bs_anc_row(p, row0 + b, row0 + b, lane);
  }
}

// The step from "finalize" on, for the `ncand` candidates (value cv, token ct, parent beam cb; LDS, written before a
// __syncthreads) of sentence s: finalize_hypos / is_finished on the first `beam` of them, then the next step's
// hypotheses (cands_to_ignore / active_mask) and their gathered rows.  act: `beam` ints of LDS, sh_new_fin: one.
__device__ __forceinline__ void bs_finish_step(const BeamStepP& p, int s, int lane, int ncand, const float* cv,
                                               const int* ct, const int* cb, int* act, int* sh_new_fin) {
  const int beam = p.beam;
  const long long row0 = (long long)s * beam;
  // ---- finalize hypotheses that end in eos among the first `beam` candidates (lane 0: in order)
  if (lane == 0) {
    int seen = 0;
    for (int c = 0; c < beam; ++c) {
      const bool is_eos = ct[c] == p.eos && cv[c] != -INFINITY && !p.ignore[s * beam + c];
      if (!is_eos) continue;
      seen = 1;
      if (p.nfin[s] < beam) {
        const int h = p.nfin[s]++;
        const long long prow = row0 + cb[c];
        int64_t* ft = p.fin_tok + ((long long)s * beam + h) * p.Ls;
        float* fp = p.fin_pos + ((long long)s * beam + h) * p.Ls;
        for (int j = 0; j < p.step; ++j) ft[j] = p.tok_in[prow * p.Lt + 1 + j];
        ft[p.step] = p.eos;
        float prev = 0.f;
        for (int j = 0; j < p.step; ++j) {
          const float cur = p.sc_in[prow * p.Ls + j];
          fp[j] = j == 0 ? cur : cur - prev;
          prev = cur;
        }
        fp[p.step] = p.step == 0 ? cv[c] : cv[c] - prev;
        float sc = cv[c];
        if (p.normalize) {
          // the reference divides by the correctly rounded power; powf is 1 ulp off for some lengths even
          // where the power is exact (41^1), so the exact cases -- 1 is the default -- do not go through it
          const float len = (float)(p.step + 1);
          sc = sc / (p.len_penalty == 1.f ? len : p.len_penalty == 0.f ? 1.f : powf(len, p.len_penalty));
        }
        p.fin_score[s * beam + h] = sc;
        p.fin_len[s * beam + h] = p.step + 1;
      }
    }
    int fin_now = 0;
    if (seen && (p.nfin[s] == beam || p.step == p.max_len)) {
      p.finished[s] = 1;
      atomicSub(p.remaining, 1);
      fin_now = 1;
    }
    *sh_new_fin = fin_now;
  }
  __syncthreads();
  if (*sh_new_fin) {
    bs_idle_rows(p, row0, lane);
    return;
  }
  // ---- the `beam` live candidates with the smallest rank (eos / ignored ones sort behind)
  if (lane == 0) {
    int n = 0;
    for (int pass = 0; pass < 2 && n < beam; ++pass)
      for (int c = 0; c < ncand && n < beam; ++c) {
        bool dead = ct[c] == p.eos && cv[c] != -INFINITY;
        if (c < beam) dead = dead || p.ignore[s * beam + c];
        if ((pass == 0) == !dead) act[n++] = c | (dead ? 0x10000 : 0);
      }
    for (int b = 0; b < beam; ++b) p.ignore[s * beam + b] = (act[b] & 0x10000) ? 1 : 0;
  }
  __syncthreads();
  for (int b = 0; b < beam; ++b) {
    const int c = act[b] & 0xffff;
    const long long prow = row0 + cb[c], nrow = row0 + b;
    for (int j = lane; j < p.Lt; j += 64) {
      int64_t t = p.tok_in[prow * p.Lt + j];
      if (j == p.step + 1) t = ct[c];
      p.tok_out[nrow * p.Lt + j] = t;
    }
    for (int j = lane; j < p.Ls; j += 64) {
      float v = p.sc_in[prow * p.Ls + j];
      if (j == p.step) v = cv[c];
      p.sc_out[nrow * p.Ls + j] = v;
    }
    if (lane == 0) p.reorder[nrow] = prow;
    bs_anc_row(p, nrow, prow, lane);
  }
}

// Host-side filling of BeamStepP from the C-ABI arguments of vs_beam_step / vs_sample_step.
static inline BeamStepP bs_params(const float* row_val, const int64_t* row_idx, const int64_t* tok_in,
                                  int64_t* tok_out, const float* sc_in, float* sc_out, uint8_t* ignore,
                                  uint8_t* finished, int* nfin, int* remaining, int64_t* fin_tok, float* fin_score,
                                  float* fin_pos, int* fin_len, int64_t* reorder, const int32_t* anc_in,
                                  int32_t* anc_out, int anc_ld, int beam, int k, int V, int step, int max_len,
                                  int eos, int normalize, float len_penalty) {
  BeamStepP p;
  p.anc_in = anc_in; p.anc_out = anc_out; p.anc_ld = anc_ld;
  p.row_val = row_val; p.row_idx = row_idx; p.tok_in = tok_in; p.tok_out = tok_out;
  p.sc_in = sc_in; p.sc_out = sc_out; p.ignore = ignore; p.finished = finished; p.nfin = nfin;
  p.remaining = remaining; p.fin_tok = fin_tok; p.fin_score = fin_score; p.fin_pos = fin_pos;
  p.fin_len = fin_len; p.reorder = reorder;
  p.beam = beam; p.k = k; p.V = V; p.step = step; p.max_len = max_len;
  p.Lt = max_len + 2; p.Ls = max_len + 1; p.eos = eos; p.normalize = normalize;
  p.len_penalty = len_penalty;
  return p;
}
