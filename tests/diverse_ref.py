"""numpy restatement of the diverse beam searches (docs/beam_search_parity.md, "Diverse beam search"; fairseq 0.10
`search.DiverseBeamSearch` / `search.DiverseSiblingsSearch` restated from their published behaviour, PARITY UNPINNED),
independent of the library.  Per sentence and step, on the rows' lists `row_val / row_idx [bsz*beam, 2*beam]` (values
`lp + cum` descending, ties towards the lowest token; what vs_beam_topk returns):

  A. groups (G, lam >= 0, mb = beam / G): group g = beams g, g+G, ... (step 0: beam g alone), groups in order.  Every
     entry (v, token) of the group's rows competes as v' = fl32(v - fl32(lam * cnt[token])), cnt = the candidates of
     groups 0..g-1 that carry the token (-inf ones included).  The group's candidates are its 2*mb best by v' descending,
     ties towards the lowest beam*V + token, each (v', token, absolute beam); candidate j*G + g is group g's j-th best.
  B. siblings (rate >= 0): step 0 is the plain beam step; later entry r of a row's list competes as
     v' = fl32(v - fl32((r + 1) * rate)) in one merge of all beam * 2*beam entries, same order.
  v' is the candidate's score.  The 2*beam candidates are not sorted again; finalize_hypos / is_finished /
  cands_to_ignore / active_mask follow as in tests/beam_step_ref.py:85-141, restated in `_tail`.

`group_candidates_full` applies rule A to whole rows of `lp + cum` instead of lists (the sufficiency test).
"""
import numpy as np

import beam_step_ref
from oracle import beam_ref

COUNTERS = ("ignored_beam", "penalty_reordered", "penalised_entries", "cross_beam_tie", "neginf_candidate", "eos_inside_beam",
            "eos_beyond_beam", "ignore_set", "idle_steps", "merges")
F32 = np.float32


def new_counters():
    return {name: 0 for name in COUNTERS}


def check_args(beam, V, G=None, lam=0.0, rate=0.0):
    if G is not None and (G < 1 or beam % G):
        raise ValueError("the groups must divide the beam")
    if not lam >= 0 or not rate >= 0:
        raise ValueError("strengths must be >= 0")
    if V - 1 < 2 * beam:
        raise ValueError("2*beam candidates need V - 1 >= 2*beam")


def _best(v, t, b, V, n, counters=None, gaps=None):
    """Indices of the n best of the entries (v, t, b): v descending, ties towards the lowest b*V + t."""
    order = np.lexsort((b.astype(np.int64) * V + t, -v.astype(np.float64)))
    if gaps is not None and order.size > n:
        kept, rej = float(v[order[n - 1]]), float(v[order[n]])
        if np.isfinite(kept):  # both -inf: decided by the index, which no rounding moves
            gaps.append(np.inf if rej == -np.inf else kept - rej)
    if counters is not None:
        nxt = order[: n + 1]
        tie = (v[nxt][1:] == v[nxt][:-1]) & np.isfinite(v[nxt][1:])
        counters["cross_beam_tie"] += int((tie & (b[nxt][1:] != b[nxt][:-1])).sum())
        counters["merges"] += 1
    return order[:n]


def _groups(rows_v, rows_t, step, V, G, lam, counters=None, gaps=None):
    """Rule A on rows_v / rows_t [beam, n] (n = 2*beam for lists, V for whole rows): (score, token, beam) [2*beam]."""
    beam = rows_v.shape[0]
    mb = beam // G
    c_sc, c_tok = np.empty(2 * beam, dtype=F32), np.empty(2 * beam, dtype=np.int64)
    c_beam = np.empty(2 * beam, dtype=np.int64)
    chosen = []  # tokens of the candidates of the groups before
    for g in range(G):
        beams = np.array([g]) if step == 0 else np.arange(g, beam, G)
        v = rows_v[beams].astype(F32).reshape(-1)
        t = rows_t[beams].astype(np.int64).reshape(-1)
        b = np.repeat(beams, rows_v.shape[1])
        if g > 0:
            cnt = np.bincount(np.asarray(chosen, dtype=np.int64), minlength=V)[t].astype(F32)
            with np.errstate(invalid="ignore"):
                vp = (v - F32(lam) * cnt).astype(F32)
            if counters is not None:
                counters["penalised_entries"] += int(((cnt > 0) & np.isfinite(v)).sum())
                plain = _best(v, t, b, V, 2 * mb)
        else:
            vp = v
        order = _best(vp, t, b, V, 2 * mb, counters, gaps)
        if g > 0 and counters is not None and not np.array_equal(order, plain):
            counters["penalty_reordered"] += 1
        c_sc[g::G], c_tok[g::G], c_beam[g::G] = vp[order], t[order], b[order]
        chosen.extend(t[order].tolist())
    return c_sc, c_tok, c_beam


def group_candidates(rv, ri, step, V, G, lam, counters=None, gaps=None):
    """One sentence's candidates from its rows' lists rv / ri [beam, 2*beam]."""
    check_args(rv.shape[0], V, G, lam)
    assert rv.shape[1] == 2 * rv.shape[0]
    return _groups(rv, ri, step, V, G, lam, counters, gaps)


def group_candidates_full(lp_plus_cum, step, G, lam):
    """Brute force: the penalty on every token of the rows `lp_plus_cum` [beam, V], no lists."""
    beam, V = lp_plus_cum.shape
    check_args(beam, V, G, lam)
    return _groups(np.asarray(lp_plus_cum, dtype=F32), np.tile(np.arange(V), (beam, 1)), step, V, G, lam)


def sibling_candidates(rv, ri, step, V, rate, counters=None, gaps=None):
    beam, k = rv.shape
    check_args(beam, V, rate=rate)
    assert k == 2 * beam
    if step == 0:
        v, t, b = rv[0].astype(F32), ri[0].astype(np.int64), np.zeros(k, dtype=np.int64)
    else:
        pen = (np.arange(1, k + 1).astype(F32) * F32(rate)).astype(F32)
        v = (rv.astype(F32) - pen[None, :]).astype(F32).reshape(-1)
        t, b = ri.astype(np.int64).reshape(-1), np.repeat(np.arange(beam), k)
    order = _best(v, t, b, V, 2 * beam, counters, gaps)
    return v[order], t[order], b[order]


def _tail(st, new, reorder, s, step, c_sc, c_tok, c_beam, eos, max_len, normalize, len_penalty, cnt):
    """tests/beam_step_ref.py:85-141 for the candidates of sentence s (2*beam of them, in the order given)."""
    beam = st["ignore"].shape[1]
    ncand = cand_size = 2 * beam
    row0 = s * beam
    ignore = st["ignore"][s].astype(bool)
    cnt["ignored_beam"] += int(ignore.sum())
    eos_mask = (c_tok == eos) & (c_sc != -np.inf)
    cnt["eos_beyond_beam"] += int(eos_mask[beam:].sum())
    cnt["neginf_candidate"] += int((c_sc == -np.inf).sum())
    eos_mask[:beam][ignore] = False
    cnt["eos_inside_beam"] += int(eos_mask[:beam].sum())
    seen = False
    for c in np.nonzero(eos_mask[:beam])[0]:
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
            score = score / F32((step + 1) ** len_penalty)
        new["fin_score"][s, h] = score
        new["fin_len"][s, h] = step + 1
    if seen and (new["nfin"][s] == beam or step == max_len):
        new["finished"][s] = 1
        new["remaining"][0] -= 1
        return
    assert step < max_len, "a sentence outlives max_len: the lists of the last step must hold eos only"
    eos_mask[:beam] = ~((~ignore) & (~eos_mask[:beam]))
    active_mask = eos_mask.astype(np.int64) * cand_size + np.arange(ncand)
    hypos = np.argsort(active_mask, kind="stable")[:beam]
    new_ignore = active_mask[hypos] >= cand_size
    assert (~new_ignore).any()
    cnt["ignore_set"] += int(new_ignore.sum())
    new["ignore"][s] = new_ignore
    parent = row0 + c_beam[hypos]
    reorder[row0: row0 + beam] = parent
    new["tok"][row0: row0 + beam] = st["tok"][parent]
    new["tok"][row0: row0 + beam, step + 1] = c_tok[hypos]
    new["sc"][row0: row0 + beam] = st["sc"][parent]
    new["sc"][row0: row0 + beam, step] = c_sc[hypos]
    if st["anc"] is not None:
        new["anc"][row0: row0 + beam, : step + 1] = st["anc"][parent, : step + 1]


def _step(st, row_val, row_idx, step, eos, max_len, normalize, len_penalty, counters, candidates):
    cnt = counters if counters is not None else new_counters()
    bsz, beam = st["ignore"].shape
    k = row_val.shape[1]
    new = {key: (None if a is None else a.copy()) for key, a in st.items()}
    reorder = np.arange(bsz * beam, dtype=np.int64)
    rv, ri = row_val.reshape(bsz, beam, k), row_idx.reshape(bsz, beam, k)
    for s in range(bsz):
        row0 = s * beam
        if st["anc"] is not None:
            new["anc"][row0: row0 + beam, step + 1] = np.arange(row0, row0 + beam)
        if st["finished"][s]:
            cnt["idle_steps"] += 1
            continue
        c_sc, c_tok, c_beam = candidates(rv[s], ri[s], cnt)
        _tail(st, new, reorder, s, step, c_sc, c_tok, c_beam, eos, max_len, normalize, len_penalty, cnt)
    return new, reorder


def group_step(st, row_val, row_idx, step, V, eos, max_len, G, lam, normalize=True, len_penalty=1.0, counters=None,
               gaps=None):
    """(new state, reorder [bsz*beam]) on the state dict of `beam_step_ref.new_state`; `st` is left unchanged."""
    return _step(st, row_val, row_idx, step, eos, max_len, normalize, len_penalty, counters,
                 lambda rv, ri, cnt: group_candidates(rv, ri, step, V, G, lam, cnt, gaps))


def sibling_step(st, row_val, row_idx, step, V, eos, max_len, rate, normalize=True, len_penalty=1.0, counters=None,
                 gaps=None):
    return _step(st, row_val, row_idx, step, eos, max_len, normalize, len_penalty, counters,
                 lambda rv, ri, cnt: sibling_candidates(rv, ri, step, V, rate, cnt, gaps))


def banned_mask(tok, step, n, vocab):
    import beam_ngram_ref

    mask = np.zeros((tok.shape[0], vocab), dtype=bool)
    for r in range(tok.shape[0]):
        ban = [t for t in beam_ngram_ref.banned_scan(tok[r], step, n) if 0 <= t < vocab]
        mask[r, ban] = True
    return mask


def search(step_logits, bsz, vocab, pad, eos, unk, beam_size=1, max_len_b=200, min_len=1, normalize_scores=True,
           len_penalty=1.0, unk_penalty=0.0, temperature=1.0, prefix_tokens=None, no_repeat_ngram_size=0,
           groups=None, strength=0.5, rate=None, counters=None, gaps=None, trace=None):
    """A whole diverse search for a batch that does not shrink, modelled on `beam_step_ref.search` (its fp32 scoring
    rules, plus the n-gram ban): `groups` = G selects rule A with `strength`, else `rate` selects rule B.  `gaps`
    receives the decidability gap of every merge (`min_gap`), `trace` the state after every step."""
    beam = min(beam_size, vocab - 1)
    max_len = max_len_b
    assert min_len <= max_len and (groups is None) != (rate is None)
    check_args(beam, vocab, groups, strength if groups is not None else 0.0, rate or 0.0)
    k = 2 * beam
    st = beam_step_ref.new_state(bsz, beam, max_len, pad, eos)
    sent_of_row = np.repeat(np.arange(bsz), beam)
    for t in range(max_len + 1):
        logits = step_logits(st["tok"][:, : t + 1], sent_of_row)
        lprobs = beam_ref.log_softmax(np.asarray(logits, dtype=F32) / F32(temperature))
        lprobs[lprobs != lprobs] = -np.inf
        lprobs[:, pad] = -np.inf
        lprobs[:, unk] -= unk_penalty
        if t >= max_len:
            lprobs[:, :eos] = -np.inf
            lprobs[:, eos + 1:] = -np.inf
        if prefix_tokens is not None and t < prefix_tokens.shape[1] and t < max_len:
            ptoks = np.repeat(np.asarray(prefix_tokens)[:, t], beam)
            assert (ptoks != eos).all(), "eos inside the prefix is outside the device search"
            keep = lprobs[np.arange(len(ptoks)), ptoks]
            pm = ptoks != pad
            lprobs[pm] = -np.inf
            lprobs[np.nonzero(pm)[0], ptoks[pm]] = keep[pm]
        elif t < min_len:
            lprobs[:, eos] = -np.inf
        if no_repeat_ngram_size:
            lprobs[banned_mask(st["tok"], t, no_repeat_ngram_size, vocab)] = -np.inf
        row_val, row_idx = beam_step_ref.row_lists(lprobs, None if t == 0 else st["sc"][:, t - 1], k)
        if groups is not None:
            st, _ = group_step(st, row_val, row_idx, t, vocab, eos, max_len, groups, strength, normalize_scores,
                               len_penalty, counters, gaps)
        else:
            st, _ = sibling_step(st, row_val, row_idx, t, vocab, eos, max_len, rate, normalize_scores, len_penalty,
                                 counters, gaps)
        if trace is not None:
            trace.append(st)
        if st["remaining"][0] == 0:
            break
    return beam_step_ref.hypotheses(st)


def min_gap(gaps):
    """The decidability of a restated search: the smallest distance between the last kept and the first rejected v'
    over all its merges.  A kernel whose values are off by less than half of it keeps the same entries."""
    return min(gaps) if gaps else np.inf
