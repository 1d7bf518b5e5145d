"""Inputs of the sampling tests (helper, not collected), shared by the CPU fixture checks (test_sample_ref.py) and the
kernel test (test_gpu_sample_token.py), with their fp64 reference computed once per vocabulary size.

Shapes: 6 rows at V = 97 (one block per row), 2049 (the first sliced V: a second slice of one token), 4099 (three
slices, V not a multiple of 4); 4 rows at 50261 (GPT-2's vocabulary with the project's added tokens: 25 slices).
Logits are randn * 4.  Every call runs at temperature 0.7 with an unk penalty; two rule variants:
  "ban":  eos banned (flags & 2), row 2 forced to token 42, a 2-gram ban from a five-token history per row -- row 1
          loses its arg-max, row 2 its forced token (an all-banned row: kept mass 0), row 0 both sides of the first
          slice boundary where V has one;
  "last": only eos allowed (flags & 1), no forcing, no ban.
"""
import numpy as np

import sample_ref as SR

SEED = 20241
TEMPERATURE, UNK_PENALTY = 0.7, 0.25
SHAPES = {97: 6, 2049: 6, 4099: 6, 50261: 4}
VARIANTS = ("ban", "last")
STEP, NGRAM, HIST_LD = 4, 2, 8


def modes(V):
    """(name, sampling_topk, sampling_topp)."""
    return [("plain", -1, -1.0), ("topk1", 1, -1.0), ("topk5", 5, -1.0), ("topk40", 40, -1.0), ("topkV", V, -1.0),
            ("topp1e-6", -1, 1e-6), ("topp0.5", -1, 0.5), ("topp0.9", -1, 0.9), ("topp1.0", -1, 1.0)]


MODE_NAMES = [m[0] for m in modes(0)]
_cache = {}


def case(V):
    """dict: x [rows, V] f32, cum [rows] f32, pad / eos / unk, and per variant: flags, forced (or None), tokens
    (history [rows, HIST_LD] i64 or None), lp (fp64 [rows, V])."""
    if V in _cache:
        return _cache[V]
    rows = SHAPES[V]
    rs = np.random.RandomState(1000 + V)
    pad, eos, unk = V - 1, V - 2, 5
    x = (rs.randn(rows, V) * 4).astype(np.float32)
    x[:, pad] = x.max(1) - 1.0  # pad would be a likely token: the mass the rules remove is far above delta, so at
    # topp = 1.0 (masses are not renormalised) the whole row's mass is clearly below topp and every token is kept
    cum = rs.randn(rows).astype(np.float32)
    c = {"x": x, "cum": cum, "pad": pad, "eos": eos, "unk": unk, "rows": rows}
    forced = np.full(rows, -1, dtype=np.int64)
    forced[2] = 42
    b = 2047 if V > 2048 else 31
    targets = [[b, b + 1], [int(np.argmax(x[1])), 7], [42, 9], [eos, 17], [3, V - 3], [11, 12]][:rows]
    tok = np.full((rows, HIST_LD), pad, dtype=np.int64)
    for r, (t1, t2) in enumerate(targets):
        tok[r, : STEP + 1] = [60, t1, 60, t2, 60]
    banned = SR.banned_mask(tok, STEP, NGRAM, V)
    assert all(banned[r, t] for r, ts in enumerate(targets) for t in ts)
    c["ban"] = {"flags": 2, "forced": forced, "tokens": tok,
                "lp": SR.lprobs(x, pad, eos, unk, UNK_PENALTY, TEMPERATURE, ban_eos=True, forced=forced,
                                banned=banned)}
    c["last"] = {"flags": 1, "forced": None, "tokens": None,
                 "lp": SR.lprobs(x, pad, eos, unk, UNK_PENALTY, TEMPERATURE, eos_only=True)}
    _cache[V] = c
    return c
