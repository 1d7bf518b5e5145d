"""One step of the reference's beam search in numpy, for a batch that does not shrink: the restatement
`vs_beam_step` (vidsitu_amd/csrc/gpt2_ops.hip) is held to, bit for bit (tests/test_gpu_beam_step.py).

It restates `oracle/beam_ref.py` lines 81-162 -- fairseq `BeamSearch.step` on the rows' top-k lists,
`finalize_hypos` / `is_finished`, and the `cands_to_ignore` / `active_mask` selection -- sentence by
sentence, with the oracle's candidate count (`min(2*beam, V - 1)` at step 0, `min(2*beam, beam*V - 1)`
later) and its tie rule (lowest `beam*V + token` first).  Where the oracle removes a finished sentence
from the batch, the sentence idles here: its tokens, scores and flags are carried over unchanged, its
rows are their own parents.  tests/test_beam_step_ref.py chains this step behind a numpy log-softmax
(`search`) and requires the oracle's hypotheses, so the restatement is anchored on the oracle and not
on the kernel.

State (a dict of numpy arrays, the device session's buffers):
  tok [bsz*beam, max_len+2] i64   sc [bsz*beam, max_len+1] f32   ignore [bsz, beam] u8
  finished [bsz] u8   nfin [bsz] i32   remaining [1] i32
  fin_tok [bsz, beam, max_len+1] i64   fin_score [bsz, beam] f32   fin_pos [bsz, beam, max_len+1] f32
  fin_len [bsz, beam] i32   anc [bsz*beam, anc_ld] i32 or None (cache row holding position j of a row)
"""
import numpy as np

from oracle import beam_ref

COUNTERS = ("ignore_set", "neginf_selected", "eos_dropped_at_cap", "finished_at_max_len", "idle_steps",
            "cross_beam_tie", "same_token_two_beams", "eos_beyond_beam", "eos_under_ignore",
            "eos_live_tie_at_boundary", "filled_over_steps", "length_one", "last_step")


def new_counters():
    return {name: 0 for name in COUNTERS}


def new_state(bsz, beam, max_len, pad, bos, anc_ld=None):
    rows = bsz * beam
    st = {"tok": np.full((rows, max_len + 2), pad, dtype=np.int64),
          "sc": np.zeros((rows, max_len + 1), dtype=np.float32),
          "ignore": np.zeros((bsz, beam), dtype=np.uint8),
          "finished": np.zeros(bsz, dtype=np.uint8),
          "nfin": np.zeros(bsz, dtype=np.int32),
          "remaining": np.full(1, bsz, dtype=np.int32),
          "fin_tok": np.full((bsz, beam, max_len + 1), pad, dtype=np.int64),
          "fin_score": np.zeros((bsz, beam), dtype=np.float32),
          "fin_pos": np.zeros((bsz, beam, max_len + 1), dtype=np.float32),
          "fin_len": np.zeros((bsz, beam), dtype=np.int32),
          "anc": None}
    st["tok"][:, 0] = bos
    if anc_ld is not None:
        st["anc"] = np.repeat(np.arange(rows, dtype=np.int32)[:, None], anc_ld, axis=1)
    return st


def step(st, row_val, row_idx, step, V, eos, max_len, normalize=True, len_penalty=1.0, counters=None):
    """(new state, reorder [bsz*beam] i64): `row_val` / `row_idx` [bsz*beam, k] are the rows' top-k
    (cumulative scores added, descending, ties towards the lowest token); `st` is left unchanged."""
    cnt = counters if counters is not None else new_counters()
    bsz, beam = st["ignore"].shape
    k = row_val.shape[1]
    cand_size = 2 * beam
    new = {key: (None if a is None else a.copy()) for key, a in st.items()}
    reorder = np.arange(bsz * beam, dtype=np.int64)
    rv, ri = row_val.reshape(bsz, beam, k), row_idx.reshape(bsz, beam, k)
    for s in range(bsz):
        row0 = s * beam
        if st["anc"] is not None:  # every row its own parent until the sentence is found to go on
            new["anc"][row0: row0 + beam, step + 1] = np.arange(row0, row0 + beam)
        if st["finished"][s]:
            cnt["idle_steps"] += 1
            continue
        # ---- BeamSearch.step: top ncand of the flattened scores (beam_ref.py:81-90)
        if step == 0:
            v, t, b = rv[s, 0], ri[s, 0], np.zeros(k, dtype=np.int64)
            ncand = min(cand_size, V - 1)
        else:
            v, t, b = rv[s].reshape(-1), ri[s].reshape(-1), np.repeat(np.arange(beam), k)
            ncand = min(cand_size, beam * V - 1)
        assert ncand <= v.size, "the rows' lists hold fewer entries than the reference keeps"
        order = np.lexsort((b * V + t, -v.astype(np.float64)))  # value descending, then beam*V + token
        nxt = order[: ncand + 1]
        tie = (v[nxt][1:] == v[nxt][:-1]) & np.isfinite(v[nxt][1:])
        cnt["cross_beam_tie"] += int((tie & (b[nxt][1:] != b[nxt][:-1])).sum())
        order = order[:ncand]
        c_sc, c_tok, c_beam = v[order], t[order], b[order]
        live_tok = c_tok[np.isfinite(c_sc)]
        cnt["same_token_two_beams"] += int(live_tok.size - np.unique(live_tok).size)

        # ---- eos among the first `beam` candidates: finalize_hypos (beam_ref.py:92-125)
        ignore = st["ignore"][s].astype(bool)
        eos_mask = (c_tok == eos) & (c_sc != -np.inf)
        cnt["eos_under_ignore"] += int((eos_mask[:beam] & ignore).sum())
        cnt["eos_beyond_beam"] += int(eos_mask[beam:].sum())
        if ncand > beam and c_sc[beam - 1] == c_sc[beam] and np.isfinite(c_sc[beam]) \
                and eos_mask[beam - 1] != eos_mask[beam]:
            cnt["eos_live_tie_at_boundary"] += 1
        eos_mask[:beam][ignore] = False
        seen = False
        had = int(st["nfin"][s])
        for c in np.nonzero(eos_mask[:beam])[0]:
            seen = True
            if new["nfin"][s] >= beam:
                cnt["eos_dropped_at_cap"] += 1
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
            cnt["length_one"] += step == 0
        if seen and (new["nfin"][s] == beam or step == max_len):  # is_finished
            cnt["finished_at_max_len"] += int(new["nfin"][s] < beam)
            cnt["last_step"] += int(step == max_len)
            cnt["filled_over_steps"] += int(0 < had < beam and new["nfin"][s] == beam)
            new["finished"][s] = 1
            new["remaining"][0] -= 1
            continue
        assert step < max_len, "a sentence outlives max_len: the lists of the last step must hold eos only"

        # ---- the next step's hypotheses: cands_to_ignore / active_mask (beam_ref.py:150-162)
        eos_mask[:beam] = ~((~ignore) & (~eos_mask[:beam]))
        active_mask = eos_mask.astype(np.int64) * cand_size + np.arange(ncand)
        hypos = np.argsort(active_mask, kind="stable")[:beam]
        new_ignore = active_mask[hypos] >= cand_size
        assert (~new_ignore).any()
        cnt["ignore_set"] += int(new_ignore.sum())
        cnt["neginf_selected"] += int((c_sc[hypos] == -np.inf).sum())
        new["ignore"][s] = new_ignore
        parent = row0 + c_beam[hypos]
        reorder[row0: row0 + beam] = parent
        new["tok"][row0: row0 + beam] = st["tok"][parent]
        new["tok"][row0: row0 + beam, step + 1] = c_tok[hypos]
        new["sc"][row0: row0 + beam] = st["sc"][parent]
        new["sc"][row0: row0 + beam, step] = c_sc[hypos]
        if st["anc"] is not None:
            new["anc"][row0: row0 + beam, : step + 1] = st["anc"][parent, : step + 1]
    return new, reorder


def hypotheses(st):
    """finalized[sent] = hypotheses best first (stable), the output format of `beam_ref.generate`."""
    out = []
    for s in range(st["nfin"].shape[0]):
        hyps = []
        for h in range(int(st["nfin"][s])):
            n = int(st["fin_len"][s, h])
            hyps.append({"tokens": st["fin_tok"][s, h, :n].copy(), "score": float(st["fin_score"][s, h]),
                         "positional_scores": st["fin_pos"][s, h, :n].copy()})
        order = np.argsort(-np.array([h["score"] for h in hyps], dtype=np.float32), kind="stable")
        out.append([hyps[i] for i in order])
    return out


def row_lists(lprobs, cum, k):
    """The rows' top-k of `lprobs + cum`, ties towards the lowest token: what vs_beam_topk returns."""
    return beam_ref.topk_lowest_index(lprobs if cum is None else lprobs + cum[:, None], k)


def search(step_logits, bsz, vocab, pad, eos, unk, beam_size=1, max_len_b=200, min_len=1,
           normalize_scores=True, len_penalty=1.0, unk_penalty=0.0, temperature=1.0, prefix_tokens=None,
           counters=None):
    """`beam_ref.generate` rebuilt from `step`: fp32 numpy scoring rules (beam_ref.py:58-79), the rows'
    top `min(2*beam, V - 1)`, one `step`; all rows are scored at every step (idle ones included)."""
    beam = min(beam_size, vocab - 1)
    max_len = max_len_b
    assert min_len <= max_len
    k = min(2 * beam, vocab - 1)
    st = new_state(bsz, beam, max_len, pad, eos)
    sent_of_row = np.repeat(np.arange(bsz), beam)
    for t in range(max_len + 1):
        logits = step_logits(st["tok"][:, : t + 1], sent_of_row)
        lprobs = beam_ref.log_softmax(np.asarray(logits, dtype=np.float32) / np.float32(temperature))
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
        row_val, row_idx = row_lists(lprobs, None if t == 0 else st["sc"][:, t - 1], k)
        st, _ = step(st, row_val, row_idx, t, vocab, eos, max_len, normalize_scores, len_penalty, counters)
        if st["remaining"][0] == 0:
            break
    return hypotheses(st)
