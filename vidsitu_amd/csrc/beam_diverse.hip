// Diverse beam search (fairseq DiverseBeamSearch / DiverseSiblingsSearch restated; docs/beam_search_parity.md,
// "Diverse beam search"): the bookkeeping of one step on the per-row top-2*beam lists of vs_beam_topk[_ngram].
// The candidates of a sentence are formed group by group (or from rank-penalised lists); everything from "finalize" on
// is vs_beam_step's code (bs_finish_step, beam_shared.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "beam_shared.h"
#include "vidsitu_hip.h"

#define BD_MAXE (BS_MAXC * BS_MAXC / 2)  // beam * k entries of a sentence, k = 2 * beam <= BS_MAXC

// One block of 64 threads per sentence.  groups >= 1: the beams g, g + G, ... are group g; the groups run in order,
// group g keeps its 2 * beam / G best entries by v' = v - strength * cnt[token], cnt = the candidates of the groups
// before that carry the token -- the (token, count) table is the candidate list itself, cnt the number of its slots
// j * G + g', g' < g, holding the token -- and its j-th best is candidate j * G + g.  groups == 0: the siblings rule,
// one merge over all beams with v' = v - (rank + 1) * rate from step 1 on.  Neither product is contracted into its
// subtraction: v' is fl32(v - fl32(penalty)), as the restatement forms it.
__global__ __launch_bounds__(64) void beam_diverse_step_kernel(BeamStepP p, int groups, float strength, float rate) {
  __shared__ float cv[BS_MAXC];
  __shared__ int ct[BS_MAXC];
  __shared__ int cb[BS_MAXC];
  __shared__ int act[BS_MAXC];
  __shared__ float ev[BD_MAXE];  // the group's entries: penalised value
  __shared__ int et[BD_MAXE];    //                      token
  __shared__ float bestv[64];
  __shared__ long long bestf[64];
  __shared__ int besti[64];
  __shared__ int sh_new_fin;
  const int s = blockIdx.x, lane = threadIdx.x;
  const int beam = p.beam, k = p.k;
  const long long row0 = (long long)s * beam;
  if (p.finished[s]) {
    bs_idle_rows(p, row0, lane);
    return;
  }
  const int G = groups > 0 ? groups : 1, mb = beam / G;
  const int nrows = p.step == 0 ? 1 : mb;  // step 0: the group's first beam only
  const int total = nrows * k, nsel = 2 * mb;
  for (int g = 0; g < G; ++g) {
    // ---- the group's entries, penalised (the candidates of the groups before are in ct: synced at their end)
    for (int le = lane; le < total; le += 64) {
      const int b = g + (le / k) * G, r = le % k;
      float v = p.row_val[(row0 + b) * k + r];
      const int tok = (int)p.row_idx[(row0 + b) * k + r];
      if (groups == 0) {
        if (p.step > 0) v = __fsub_rn(v, __fmul_rn((float)(r + 1), rate));
      } else if (g > 0) {
        int cnt = 0;
        for (int j = 0; j < nsel; ++j)
          for (int q = 0; q < g; ++q) cnt += ct[j * G + q] == tok;
        v = __fsub_rn(v, __fmul_rn(strength, (float)cnt));
      }
      ev[le] = v; et[le] = tok;
    }
    __syncthreads();
    // ---- its nsel best, by v' descending, ties towards the lowest beam*V + token: beam_step_kernel's loop
    float pv = INFINITY;
    long long pf = -1;
    for (int j = 0; j < nsel; ++j) {
      float bv = -INFINITY;
      long long bf = 0x7fffffffffffffffll;
      int bi = -1;
      for (int le = lane; le < total; le += 64) {
        const float v = ev[le];
        const long long f = (long long)(g + (le / k) * G) * p.V + et[le];
        const bool after = (v < pv) || (v == pv && f > pf);
        if (after && (v > bv || (v == bv && f < bf))) { bv = v; bf = f; bi = le; }
      }
      bestv[lane] = bv; bestf[lane] = bf; besti[lane] = bi;
      __syncthreads();
      for (int st = 32; st > 0; st >>= 1) {
        if (lane < st) {
          const float v2 = bestv[lane + st]; const long long f2 = bestf[lane + st];
          if (besti[lane + st] >= 0 && (besti[lane] < 0 || v2 > bestv[lane] || (v2 == bestv[lane] && f2 < bestf[lane]))) {
            bestv[lane] = v2; bestf[lane] = f2; besti[lane] = besti[lane + st];
          }
        }
        __syncthreads();
      }
      if (lane == 0) {
        const int c = j * G + g;
        if (besti[0] >= 0) {
          cv[c] = bestv[0]; ct[c] = et[besti[0]]; cb[c] = g + (besti[0] / k) * G;
        } else {  // unreachable: a row's list holds k = 2*beam >= nsel distinct tokens; keeps cv/ct/cb defined
          cv[c] = -INFINITY; ct[c] = 0; cb[c] = g;
        }
      }
      pv = bestv[0]; pf = bestf[0];
      __syncthreads();
    }
  }
  bs_finish_step(p, s, lane, 2 * beam, cv, ct, cb, act, &sh_new_fin);
}

extern "C" int vs_beam_diverse_step(const float* row_val, const int64_t* row_idx, const int64_t* tok_in,
                                    int64_t* tok_out, const float* sc_in, float* sc_out, uint8_t* ignore,
                                    uint8_t* finished, int* nfin, int* remaining, int64_t* fin_tok, float* fin_score,
                                    float* fin_pos, int* fin_len, int64_t* reorder, const int32_t* anc_in,
                                    int32_t* anc_out, int anc_ld, int bsz, int beam, int k, int V, int step,
                                    int max_len, int eos, int normalize, float len_penalty, int groups,
                                    float strength, float sibling_rate, void* stream) {
  VS_CHECK_ARG(row_val && row_idx && tok_in && tok_out && sc_in && sc_out && ignore && finished && nfin &&
                   remaining && fin_tok && fin_score && fin_pos && fin_len && reorder, "null argument");
  VS_CHECK_ARG(bsz > 0 && beam >= 1 && 2 * beam <= BS_MAXC, "beam <= 32");
  VS_CHECK_ARG(k == 2 * beam && 2 * beam <= V - 1, "a diverse search needs lists of k = 2*beam <= V - 1 entries");
  VS_CHECK_ARG(step >= 0 && step <= max_len, "step must be in [0, max_len]");
  VS_CHECK_ARG(groups >= 0 && (groups == 0 || beam % groups == 0), "groups must divide beam (0: siblings)");
  // !(x >= 0) also refuses NaN
  VS_CHECK_ARG(strength >= 0.f && sibling_rate >= 0.f, "diversity strength / rate must be >= 0");
  VS_CHECK_ARG(groups == 0 || sibling_rate == 0.f, "groups and a sibling rate exclude each other");
  VS_CHECK_ARG((anc_in == nullptr) == (anc_out == nullptr) && (!anc_out || anc_ld > step), "ancestry tables");
  const BeamStepP p = bs_params(row_val, row_idx, tok_in, tok_out, sc_in, sc_out, ignore, finished, nfin, remaining,
                                fin_tok, fin_score, fin_pos, fin_len, reorder, anc_in, anc_out, anc_ld, beam, k, V,
                                step, max_len, eos, normalize, len_penalty);
  hipLaunchKernelGGL(beam_diverse_step_kernel, dim3(bsz), dim3(64), 0, (hipStream_t)stream, p, groups, strength,
                     sibling_rate);
  VS_CHECK_LAUNCH();
  return VS_OK;
}
