"""numpy fp64 restatement of the sampling search (docs/beam_search_parity.md, "Sampling"; fairseq `search.Sampling`
restated from its published behaviour, PARITY UNPINNED), independent of the library:

  1. lp_j: the scoring rules of a beam-search step (oracle/beam_ref.py:58-79 plus the n-gram ban), p_j = exp(lp_j),
     not renormalised;
  2. kept set: tokens ranked by (lp descending, token ascending); plain keeps p_j > 0, top-k the first min(k, V),
     nucleus the first n + 1 (capped at V) with n = number of ranked prefixes whose cumulative p is < topp;
  3. draw: u = (w + 0.5) * 2^-32, w = tests/dropout_ref.words(seed, step, SAMPLE_SITE, row id); the token is the
     inverse CDF at u * S over the kept set in ascending token id, S the kept mass;
  4. one candidate per row: (lp_token + cum[row], token); S = 0 gives (-inf, lowest token id);
  5. candidate c of a sentence is (parent beam c, row c's draw): no merge, no sorting; finalize_hypos / is_finished /
     cands_to_ignore / active_mask as in tests/beam_step_ref.py with beam candidates per sentence.
"""
import numpy as np

import beam_ngram_ref
import beam_step_ref
import dropout_ref

SAMPLE_SITE = 0x53414D50
DELTA = 1e-5  # the tests' slack on a CDF position, as a fraction of the kept mass (derivation: the parity document)


def lprobs(logits, pad, eos, unk, unk_penalty=0.0, temperature=1.0, eos_only=False, ban_eos=False, forced=None,
           banned=None):
    """fp64 lp [rows, V] of fp32 logits.  forced: int [rows] or None (< 0 or pad: not forced); banned: bool
    [rows, V] or None (the n-gram ban)."""
    x = np.asarray(logits, dtype=np.float64) / np.float64(temperature)
    m = x.max(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))
    lp[lp != lp] = -np.inf
    lp[:, pad] = -np.inf
    lp[:, unk] -= unk_penalty
    if eos_only:
        lp[:, :eos] = -np.inf
        lp[:, eos + 1:] = -np.inf
    if forced is not None:
        forced = np.asarray(forced)
        for r in np.nonzero((forced >= 0) & (forced != pad))[0]:
            keep = lp[r, forced[r]]
            lp[r] = -np.inf
            lp[r, forced[r]] = keep
    if ban_eos:
        rows = np.ones(lp.shape[0], dtype=bool) if forced is None else ~((np.asarray(forced) >= 0) & (forced != pad))
        lp[rows, eos] = -np.inf
    if banned is not None:
        lp[banned] = -np.inf
    return lp


def banned_mask(tok, step, n, vocab):
    """bool [rows, V]: the tokens the n-gram ban removes from every row at `step` (beam_ngram_ref.banned_scan)."""
    mask = np.zeros((tok.shape[0], vocab), dtype=bool)
    for r in range(tok.shape[0]):
        ban = [t for t in beam_ngram_ref.banned_scan(tok[r], step, n) if 0 <= t < vocab]
        mask[r, ban] = True
    return mask


def ranked(lp_row):
    """Token ids of one row by (lp descending, token ascending)."""
    return np.lexsort((np.arange(lp_row.size), -lp_row))


def kept_set(lp_row, sampling_topk=-1, sampling_topp=-1.0):
    """bool [V]: the kept tokens of one row."""
    assert not (sampling_topk > 0 and sampling_topp > 0)
    v = lp_row.size
    p = np.exp(lp_row)
    keep = np.zeros(v, dtype=bool)
    if sampling_topk > 0:
        keep[ranked(lp_row)[: min(int(sampling_topk), v)]] = True
    elif sampling_topp > 0:
        order = ranked(lp_row)
        n = int((np.cumsum(p[order]) < sampling_topp).sum())
        keep[order[: min(n + 1, v)]] = True
    else:
        keep = p > 0
    return keep


def nucleus_margin(lp_row, topp):
    """Distance of `topp` from the cumulative masses on either side of the nucleus boundary -- (topp - cum_n,
    cum_{n+1} - topp) -- and the mass ranked behind the kept set.  A kernel whose sums are off by less than the
    smaller distance keeps the same set; where every token is kept or the mass behind is negligible, a different cut
    cannot change a draw by more than that mass."""
    order = ranked(lp_row)
    cum = np.cumsum(np.exp(lp_row)[order])
    n = int((cum < topp).sum())
    below = topp - (cum[n - 1] if n > 0 else 0.0)
    above = (cum[n] - topp) if n < cum.size else np.inf
    behind = cum[-1] - cum[min(n, cum.size - 1)]
    return below, above, behind


def cdf(lp_row, keep):
    """(F_lo [V], F_hi [V], S): the interval of every token on the kept masses' running sum in ascending token id
    (an empty interval for a token that is not kept)."""
    mass = np.where(keep, np.exp(lp_row), 0.0)
    hi = np.cumsum(mass)
    return hi - mass, hi, float(hi[-1])


def uniforms(seed, step, row_ids):
    w = dropout_ref.words(seed, step, SAMPLE_SITE, np.asarray(row_ids, dtype=np.uint64))
    return (w.astype(np.float64) + 0.5) / 4294967296.0


def draw_row(lp_row, keep, u):
    """(lp of the drawn token, token): the inverse CDF at u * S; S = 0 -> (-inf, lowest token id)."""
    lo, hi, s = cdf(lp_row, keep)
    if s == 0.0:
        return -np.inf, 0
    t = int(np.searchsorted(hi, u * s, side="right"))
    t = min(t, lp_row.size - 1)
    while not (keep[t] and hi[t] > lo[t]):  # u * S on the last boundary by rounding: the last kept token
        t -= 1
    return float(lp_row[t]), t


def draw(lp, cum, u, sampling_topk=-1, sampling_topp=-1.0):
    """One candidate per row: (value f32 [rows], token i64 [rows])."""
    rows = lp.shape[0]
    val, tok = np.empty(rows, dtype=np.float32), np.empty(rows, dtype=np.int64)
    for r in range(rows):
        v, t = draw_row(lp[r], kept_set(lp[r], sampling_topk, sampling_topp), u[r])
        val[r] = np.float32(v + (0.0 if cum is None else float(cum[r])))
        tok[r] = t
    return val, tok


def step(st, val, tok, step, eos, max_len, normalize=True, len_penalty=1.0):
    """(new state, reorder): rule 5 on the state dict of `beam_step_ref.new_state`; val / tok [bsz*beam] are the rows'
    draws.  Everything from finalize_hypos on restates beam_step_ref.step with `beam` candidates."""
    bsz, beam = st["ignore"].shape
    new = {key: (None if a is None else a.copy()) for key, a in st.items()}
    reorder = np.arange(bsz * beam, dtype=np.int64)
    for s in range(bsz):
        row0 = s * beam
        if st["anc"] is not None:
            new["anc"][row0: row0 + beam, step + 1] = np.arange(row0, row0 + beam)
        if st["finished"][s]:
            continue
        c_sc, c_tok, c_beam = val[row0: row0 + beam], tok[row0: row0 + beam], np.arange(beam)
        ignore = st["ignore"][s].astype(bool)
        eos_mask = (c_tok == eos) & (c_sc != -np.inf)
        eos_mask[ignore] = False
        seen = False
        for c in np.nonzero(eos_mask)[0]:
            seen = True
            if new["nfin"][s] >= beam:
                continue
            h = int(new["nfin"][s])
            new["nfin"][s] += 1
            prow = row0 + int(c_beam[c])
            new["fin_tok"][s, h, :step] = st["tok"][prow, 1: step + 1]
            new["fin_tok"][s, h, step] = eos
            pos = st["sc"][prow, : step + 1].copy()
            pos[step] = c_sc[c]
            pos[1:] = pos[1:] - pos[:-1]
            new["fin_pos"][s, h, : step + 1] = pos
            score = c_sc[c]
            if normalize:
                score = score / np.float32((step + 1) ** len_penalty)
            new["fin_score"][s, h] = score
            new["fin_len"][s, h] = step + 1
        if seen and (new["nfin"][s] == beam or step == max_len):
            new["finished"][s] = 1
            new["remaining"][0] -= 1
            continue
        assert step < max_len, "a sentence outlives max_len: the last step must draw eos"
        dead = ~((~ignore) & (~eos_mask))
        active_mask = dead.astype(np.int64) * (2 * beam) + np.arange(beam)
        hypos = np.argsort(active_mask, kind="stable")[:beam]
        new["ignore"][s] = active_mask[hypos] >= 2 * beam
        parent = row0 + c_beam[hypos]
        reorder[row0: row0 + beam] = parent
        new["tok"][row0: row0 + beam] = st["tok"][parent]
        new["tok"][row0: row0 + beam, step + 1] = c_tok[hypos]
        new["sc"][row0: row0 + beam] = st["sc"][parent]
        new["sc"][row0: row0 + beam, step] = c_sc[hypos]
        if st["anc"] is not None:
            new["anc"][row0: row0 + beam, : step + 1] = st["anc"][parent, : step + 1]
    return new, reorder


def search(step_logits, bsz, vocab, pad, eos, unk, seed, step0=0, beam_size=1, max_len_b=200, min_len=1,
           normalize_scores=True, len_penalty=1.0, unk_penalty=0.0, temperature=1.0, prefix_tokens=None,
           sampling_topk=-1, sampling_topp=-1.0, no_repeat_ngram_size=0, trace=None):
    """A whole sampling search for a batch that does not shrink: search step t draws with the generator words of
    (seed, step0 + t).  step_logits(tokens [rows, t+1], sent_ids [rows]) -> logits [rows, V].  Returns
    (hypotheses best first, number of steps run); `trace` receives (lp, cum, u, val, tok) of every step."""
    beam = min(beam_size, vocab - 1)
    max_len = max_len_b
    assert min_len <= max_len
    st = beam_step_ref.new_state(bsz, beam, max_len, pad, eos)
    sent_of_row = np.repeat(np.arange(bsz), beam)
    nsteps = 0
    for t in range(max_len + 1):
        logits = step_logits(st["tok"][:, : t + 1], sent_of_row)
        forced, ban_eos = None, False
        if prefix_tokens is not None and t < prefix_tokens.shape[1] and t < max_len:
            forced = np.repeat(np.asarray(prefix_tokens)[:, t], beam)
        elif t < min_len:
            ban_eos = True
        banned = None
        if no_repeat_ngram_size:
            banned = banned_mask(st["tok"], t, no_repeat_ngram_size, vocab)
        lp = lprobs(logits, pad, eos, unk, unk_penalty, temperature, eos_only=t >= max_len, ban_eos=ban_eos,
                    forced=forced, banned=banned)
        cum = None if t == 0 else st["sc"][:, t - 1]
        u = uniforms(seed, step0 + t, np.arange(bsz * beam))
        val, tok = draw(lp, cum, u, sampling_topk, sampling_topp)
        if trace is not None:
            trace.append((lp, cum, u, val, tok))
        st, _ = step(st, val, tok, t, eos, max_len, normalize_scores, len_penalty)
        nsteps += 1
        if st["remaining"][0] == 0:
            break
    return beam_step_ref.hypotheses(st), nsteps
