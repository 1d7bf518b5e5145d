"""Reference side of the n-gram blocking tests (helper, not collected): the reference's
`SeqGenCustom._no_repeat_ngram` / `calculate_banned_tokens` (`vidsitu_code/seq_gen.py:718-772`) restated
for one row, the scan the HIP kernel makes instead, and the oracle search with the ban put in.

Placement: the reference bans after NaN -> -inf, pad, unk penalty, max-len, prefix forcing and min-len
(`:332-353`, then `:374`) and before the search step.  The ban and every one of those rules except the
unk penalty only write -inf; the penalty subtracts a finite number and -inf - c = -inf.  So the ban
commutes with all of them and may be written right after the log-softmax, which is where `generate`
below puts it (the one exception, the eos-in-prefix beam copy, is not used here).
"""
from unittest import mock

import numpy as np

from oracle import beam_ref


def banned_ref(row, step, n):
    """`:739-772` for one full row (pad tail included): dict of comma-joined (n-1)-gram keys -> followers,
    looked up with the last n-1 tokens.  Returns the list of banned tokens, duplicates kept."""
    gen_tokens = [int(t) for t in row]
    lst = [gen_tokens[i:] for i in range(n)]
    min_len = min(len(x) for x in lst)
    gen_ngrams = {}
    for ngram in [[r[i] for r in lst] for i in range(min_len)]:
        key = ",".join(str(x) for x in ngram[:-1])
        gen_ngrams[key] = gen_ngrams.get(key, []) + [ngram[-1]]
    if step + 2 - n >= 0:
        tokens_list = gen_tokens[step + 2 - n: step + 1]
        return gen_ngrams.get(",".join(str(x) for x in tokens_list), [])
    return []


def banned_scan(row, step, n):
    """Positions 0..step only: every start i of an earlier (n-1)-gram whose follower row[i+n-1] lies at
    or before `step`, compared with the suffix row[step+2-n .. step]."""
    s0 = step + 2 - n
    out = []
    for i in range(max(s0, 0)):
        if all(int(row[i + j]) == int(row[s0 + j]) for j in range(n - 1)):
            out.append(int(row[i + n - 1]))
    return out


def live(banned, pad):
    return sorted(set(int(t) for t in banned if int(t) != pad))


def generate(step_logits, no_repeat_ngram_size, **kw):
    """`oracle.beam_ref.generate(step_logits, **kw)`, unchanged, with n-gram blocking: for the duration
    of the call `beam_ref.log_softmax` also writes -inf at each row's banned tokens (`banned_ref` on
    the row the step callback just saw, pad-filled to the oracle's full width), and
    `beam_ref.topk_lowest_index` is watched (its result is passed through).
    Returns (finalized, live_bans, min_gap):
      live_bans = number of (step, row, token != pad) bans applied;
      min_gap   = smallest difference of two adjacent finite values among the k + 1 best scores of each
                  row the search's top-k sees (all beams of a sentence, cumulative scores added), over
                  all steps -- how far the search is from a choice that rounding could turn."""
    n = int(no_repeat_ngram_size)
    pad = kw["pad"]
    max_len = min(int(kw.get("max_len_a", 0) * kw.get("src_len", 1) + kw.get("max_len_b", 200)),
                  kw.get("max_decoder_positions", 1024) - 1)
    seen = {}
    stats = {"bans": 0, "gap": np.inf}

    def cb(tokens, sent_ids):
        seen["tokens"] = np.array(tokens, copy=True)
        return step_logits(tokens, sent_ids)

    plain_lsm, plain_topk = beam_ref.log_softmax, beam_ref.topk_lowest_index

    def banned_log_softmax(x, *dtype):
        lp = plain_lsm(x, *dtype)
        toks = seen["tokens"]
        step = toks.shape[1] - 1
        for r in range(lp.shape[0] if n > 0 else 0):
            row = np.full(max_len + 2, pad, dtype=np.int64)
            row[: step + 1] = toks[r]
            ban = live(banned_ref(row, step, n), pad)
            stats["bans"] += len(ban)
            lp[r, ban] = -np.inf
        return lp

    def watched_topk(v, k):
        for top in plain_topk(v, min(k + 1, v.shape[1]))[0]:
            top = top[np.isfinite(top)]
            if top.size > 1:
                stats["gap"] = min(stats["gap"], float(np.min(top[:-1] - top[1:])))
        return plain_topk(v, k)

    with mock.patch.object(beam_ref, "log_softmax", banned_log_softmax), \
            mock.patch.object(beam_ref, "topk_lowest_index", watched_topk):
        fin = beam_ref.generate(cb, **kw)
    return fin, stats["bans"], stats["gap"]


def has_repeated_ngram(tokens, n):
    """True if the sequence holds the same n consecutive tokens twice."""
    grams = [tuple(int(t) for t in tokens[i: i + n]) for i in range(len(tokens) - n + 1)]
    return len(grams) != len(set(grams))


def stub_tables(V, seed, bsz):
    """Tables of the stub decoder and its forced first tokens, drawn in this order.  The next-token
    logits depend on the last token and on a hash of the whole history: a first-order table alone
    gives beams that end in the same token exactly tied continuations."""
    rs = np.random.RandomState(seed)
    table = (rs.randn(V, V) * 2).astype(np.float32)
    hist = rs.randn(101, V).astype(np.float32)
    prefix = rs.randint(4, V, (bsz, 1)).astype(np.int64)
    return table, hist, prefix


def stub_step_logits(table, hist):
    def step_logits(tokens, sent_ids):
        h = (tokens * np.arange(1, tokens.shape[1] + 1, dtype=np.int64)).sum(1) % 101
        return table[tokens[:, -1]] + hist[h]

    return step_logits
