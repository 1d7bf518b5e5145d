"""Scripted inputs of the beam-search tests, shared by the CPU checks (tests/test_beam_step_ref.py) and
the GPU tests (tests/test_gpu_beam_step.py): the candidate lists of the step-level comparison, and the
table-lookup decoder of the whole-search comparison, once in numpy and once in torch."""
import numpy as np

import beam_step_ref as S
from oracle import beam_ref

GRID = 2.0 ** -6


# ---- step level: lists on an exact grid ----------------------------------------------------------------
# name: bsz, beam, V, max_len, min_len, normalize, len_penalty, anc (None | extra columns over Lt), then the
# generator's knobs: levels = number of distinct table values (few: many ties), p_eos = chance that a row's
# eos gets the row's best value, p_dead = chance that a non-eos token scores -inf, narrow = steps at which
# only token 0 of a sentence's first beam is finite (every other hypothesis of the next step is a -inf one), seed; and `expect`, the
# counters of the restatement that this case is there to raise (tests/test_beam_step_ref.py asserts them)
def _c(bsz, beam, V, max_len, min_len=0, normalize=True, len_penalty=1.0, anc=0, levels=512, p_eos=0.1,
       p_dead=0.0, narrow=(), seed=0, expect=()):
    return dict(bsz=bsz, beam=beam, V=V, max_len=max_len, min_len=min_len, normalize=normalize,
                len_penalty=len_penalty, anc=anc, levels=levels, p_eos=p_eos, p_dead=p_dead, narrow=narrow,
                seed=seed, expect=expect)


_TIES = ("cross_beam_tie", "same_token_two_beams", "eos_live_tie_at_boundary")
STEP_CASES = {
    "beam1_bsz1": _c(1, 1, 9, 9, levels=4, p_eos=0.15, anc=None, expect=("idle_steps",)),
    "beam1_bsz7": _c(7, 1, 3, 12, levels=8, p_eos=0.2, len_penalty=0.5, expect=("idle_steps", "length_one")),
    "beam32_bsz1": _c(1, 32, 80, 14, min_len=1, levels=24, p_eos=0.25, anc=3,
                      expect=_TIES + ("eos_dropped_at_cap", "eos_beyond_beam", "filled_over_steps")),
    "beam32_bsz7": _c(7, 32, 65, 12, levels=16, p_eos=0.4, normalize=False, seed=1,
                      expect=_TIES + ("eos_dropped_at_cap", "eos_beyond_beam", "idle_steps")),
    "beam17_bsz2": _c(2, 17, 40, 9, levels=6, p_eos=0.3, len_penalty=2.0, anc=None, seed=2, expect=_TIES),
    "tiny_V4_beam3": _c(7, 3, 4, 9, levels=3, p_eos=0.4, p_dead=0.3, seed=3,
                        expect=("ignore_set", "neginf_selected", "eos_under_ignore", "length_one")),
    "tiny_V4_beam3_min2": _c(7, 3, 4, 8, min_len=2, levels=4, p_eos=0.3, anc=None, len_penalty=0.5, seed=4,
                             expect=("neginf_selected",)),
    "tiny_V4_beam3_to_max_len": _c(7, 3, 4, 6, min_len=6, levels=4, normalize=False, narrow=(5,), seed=4,
                                   expect=("neginf_selected", "finished_at_max_len")),
    "tiny_V5_beam4": _c(7, 4, 5, 10, levels=4, p_eos=0.4, p_dead=0.3, anc=2, seed=5,
                        expect=("ignore_set", "neginf_selected", "eos_under_ignore")),
    "tiny_V7_beam5": _c(7, 5, 7, 10, levels=5, p_eos=0.3, p_dead=0.3, len_penalty=2.0, seed=6,
                        expect=("neginf_selected",)),
    "eos_heavy": _c(7, 5, 12, 24, levels=6, p_eos=0.5, seed=7,
                    expect=_TIES + ("eos_dropped_at_cap", "filled_over_steps", "eos_beyond_beam", "idle_steps")),
    "eos_heavy_dead": _c(7, 4, 10, 22, min_len=1, levels=5, p_eos=0.35, p_dead=0.5, normalize=False,
                         anc=None, seed=8, expect=("eos_dropped_at_cap", "idle_steps")),
    "eos_rare_idle": _c(7, 3, 30, 30, levels=64, p_eos=0.12, anc=1, seed=9, expect=("idle_steps",)),
    "Lt64": _c(2, 3, 20, 62, min_len=60, levels=16, p_eos=0.3, seed=10, expect=("last_step",)),
    "Lt65": _c(2, 3, 20, 63, min_len=30, levels=16, p_eos=0.05, anc=4, seed=11, expect=("idle_steps",)),
    "Lt72": _c(3, 2, 20, 70, min_len=69, levels=16, p_eos=0.3, len_penalty=0.5, narrow=(0, 69), seed=12,
               expect=("finished_at_max_len", "last_step")),
    "Lt72_no_anc": _c(2, 4, 11, 70, min_len=50, levels=8, p_eos=0.04, anc=None, seed=13, expect=("idle_steps",)),
    "config_len200": _c(8, 5, 50, 200, min_len=160, levels=32, p_eos=0.025, seed=16,
                        expect=_TIES + ("idle_steps", "last_step")),
}
# sentences that idle for >= 10 steps while others run: asserted for these
LONG_IDLE = ("eos_rare_idle", "config_len200")


class ScriptedLists:
    """Per step and row a score table of multiples of 2^-6 in [-8, 0], plus the row's cumulative score;
    the scoring rules a search applies (pad = -inf, eos banned below min_len, only eos at max_len); then
    the row's top k with `beam_ref.topk_lowest_index`.  Every sum is a multiple of 2^-6 below 2^11 (at
    most 201 steps of at most 8), hence exact in fp32: ties are real ties, on both sides."""

    def __init__(self, case):
        self.c = case
        self.rs = np.random.RandomState(1000 + case["seed"])
        V, beam = case["V"], case["beam"]
        self.pad, self.eos = V - 1, V - 2
        self.k = min(2 * beam, V - 1)
        # the values a table may hold: `levels` of them, spread over [-8, 0]
        self.values = -GRID * np.unique(self.rs.randint(0, 513, size=case["levels"])).astype(np.float32)

    def lists(self, step, cum):
        c, rs = self.c, self.rs
        rows, V = c["bsz"] * c["beam"], c["V"]
        tab = self.values[rs.randint(0, self.values.size, size=(rows, V))]
        dead = rs.rand(rows, V) < c["p_dead"]
        dead[:, self.eos] = False
        dead[:, 0] = False  # one live token per row, so that a sentence can always go on
        tab[dead] = -np.inf
        if step in c["narrow"]:
            tab[:, 1:] = -np.inf
            tab.reshape(c["bsz"], c["beam"], V)[:, 1:] = -np.inf
        boost = rs.rand(rows) < c["p_eos"]
        tab[boost, self.eos] = self.values.max()
        if step % 3 == 1:  # the beams of a sentence share one table: the same token, equal gains
            tab = np.repeat(tab.reshape(c["bsz"], c["beam"], V)[:, :1], c["beam"], axis=1).reshape(rows, V)
        tab[:, self.pad] = -np.inf
        if step >= c["max_len"]:
            tab[:, : self.eos] = -np.inf
            tab[:, self.eos + 1:] = -np.inf
        elif step < c["min_len"]:
            tab[:, self.eos] = -np.inf
        assert np.all(np.abs(tab[np.isfinite(tab)]) <= 8) and np.all(tab[np.isfinite(tab)] % GRID == 0)
        return S.row_lists(tab, None if step == 0 else cum, self.k)


# what the finalised-hypothesis buffers hold before a step-level comparison: slots that were never written
# must still hold it afterwards
SENTINEL = {"fin_tok": -7, "fin_score": 123.5, "fin_pos": -99.25, "fin_len": -3}


def run_step_case(case, counters=None, on_step=None, on_start=None):
    """Chains the restatement over a case's scripted lists, the finalised-hypothesis buffers pre-filled
    with SENTINEL.  `on_start(state)` sees the initial state, `on_step(step, row_val, row_idx, state,
    reorder)` every step's lists and what they produced.  Returns the final state."""
    c = case
    gen = ScriptedLists(c)
    Lt = c["max_len"] + 2
    st = S.new_state(c["bsz"], c["beam"], c["max_len"], gen.pad, gen.eos,
                     None if c["anc"] is None else Lt + c["anc"])
    for key, value in SENTINEL.items():
        st[key][:] = value
    if on_start is not None:
        on_start(st)
    for step in range(c["max_len"] + 1):
        row_val, row_idx = gen.lists(step, st["sc"][:, step - 1] if step else None)
        st, reorder = S.step(st, row_val, row_idx, step, c["V"], gen.eos, c["max_len"], c["normalize"],
                             c["len_penalty"], counters)
        if on_step is not None:
            on_step(step, row_val, row_idx, st, reorder)
    assert st["remaining"][0] == 0 and st["finished"].all()
    return st


# ---- whole searches: a decoder that looks its logits up by a hash of the row's full history ------------
HASH_A, HASH_B = 251, 257


def hash_weights(length):
    """w_j of h = sum_j (token_j + 1) * w_j mod (251 * 257): fixed pseudo-random multipliers per position."""
    return np.random.RandomState(77).randint(1, HASH_A * HASH_B, size=length).astype(np.int64)


def hash_tables(V, seed, scale=10.0, eos=2, eos_bias=0.0):
    """Two tables on a 0.25 grid, logits = A[h % 251] + B[h // 251]: exact in fp32, 64 507 distinct rows."""
    rs = np.random.RandomState(seed)
    a = np.round(rs.randn(HASH_A, V) * scale * 4 / 1.5) / 4
    b = np.round(rs.randn(HASH_B, V) * scale * 4 / 3) / 4
    a[:, eos] += eos_bias
    return a.astype(np.float32), b.astype(np.float32)


def hash_step_logits(a, b, weights):
    def f(tokens, sent_ids):
        h = ((tokens + 1) * weights[: tokens.shape[1]]).sum(1) % (HASH_A * HASH_B)
        return a[h % HASH_A] + b[h // HASH_A]
    return f


# name: oracle keywords + table knobs.  pad 1, eos 2, unk 3 (V >= 4).  Seeds are chosen on the CPU so that
# the conditions of tests/test_beam_step_ref.py hold; no case may be skipped.
def _s(V, beam, bsz, max_len_b, min_len=1, seed=0, scale=10.0, eos_bias=0.0, prefix_len=0, **kw):
    return dict(V=V, beam=beam, bsz=bsz, max_len_b=max_len_b, min_len=min_len, seed=seed, scale=scale,
                eos_bias=eos_bias, prefix_len=prefix_len, kw=kw)


SEARCH_CASES = {
    "len70_beam16": _s(40, 16, 3, 70, min_len=40, seed=11),
    "len200_beam5_min199": _s(50, 5, 8, 200, min_len=199, seed=0),
    "min_len_eq_max_len": _s(30, 4, 3, 12, min_len=12, seed=0),
    "prefix_as_long_as_max_len": _s(30, 3, 3, 6, min_len=0, seed=0, prefix_len=6),
    "unnormalized": _s(30, 4, 3, 16, seed=0, eos_bias=8.0, normalize_scores=False),
    "len_penalty_half": _s(30, 4, 3, 16, seed=0, eos_bias=8.0, len_penalty=0.5),
    "V2049": _s(2049, 5, 2, 12, seed=0, eos_bias=12.0),
    "tiny_V4_beam3": _s(4, 3, 3, 7, min_len=0, seed=0, scale=1.0),
    "tiny_V5_beam4": _s(5, 4, 3, 7, min_len=1, seed=0, scale=1.0),
    "tiny_V7_beam5": _s(7, 5, 3, 7, min_len=2, seed=0, scale=1.0),
}


def search_inputs(case):
    """(tables a, b, hash weights, prefix or None, keywords of beam_ref.generate / S.search)."""
    c = case
    a, b = hash_tables(c["V"], 500 + c["seed"], c["scale"], eos=2, eos_bias=c["eos_bias"])
    prefix = None
    if c["prefix_len"]:
        rs = np.random.RandomState(c["seed"])
        prefix = np.where(rs.rand(c["bsz"], c["prefix_len"]) < 0.3, 1, 3 + rs.randint(0, c["V"] - 3, size=(
            c["bsz"], c["prefix_len"]))).astype(np.int64)
    kw = dict(bsz=c["bsz"], vocab=c["V"], pad=1, eos=2, unk=3, beam_size=c["beam"], max_len_b=c["max_len_b"],
              min_len=c["min_len"], unk_penalty=0.3, prefix_tokens=prefix, **c["kw"])
    return a, b, hash_weights(c["max_len_b"] + 2), prefix, kw


_oracle_cache = {}


def search_oracle(name):
    """The oracle's fp32 hypotheses of a whole-search case, computed once."""
    if name not in _oracle_cache:
        a, b, w, prefix, kw = search_inputs(SEARCH_CASES[name])
        _oracle_cache[name] = beam_ref.generate(hash_step_logits(a, b, w), **kw)
    return _oracle_cache[name]


# ---- vs_beam_topk where its dispatch turns -------------------------------------------------------------
TOPK_V = [2, 11, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 6145]
TOPK_BIG = [(65536, 32), (65537, 32), (65537, 31)]  # sliced with S*k = 1024 / one block per row / sliced, 1023
TOPK_T = (1.0, 0.7)
UNK_PENALTY = 0.3
SPECIALS = 8  # kinds of row, by r % 8


def topk_shapes(V):
    """(k, rows per call, rows in all) of one small V."""
    return [(k, rows, 160 if rows == 160 else SPECIALS) for k in (1, 10, 32) if k < V for rows in (1, 160)]


def topk_kmax(V):
    """The largest k any test asks of this V."""
    return max([k for k in (1, 10, 32) if k < V] if V in TOPK_V else [k for v, k in TOPK_BIG if v == V])


def topk_inputs(V, total):
    """Logits on a 0.25 grid [total, V], cum [total], forced [total], pad, eos, unk.  Row r is of kind
    r % 8: 0 ties (the row's best value at tokens 255 | 256 and 2047 | 2048 where they exist, else at the
    last two live tokens), 1 a NaN logit, 2 a forced token, 3 forced == pad, 4 cum = -inf, 5 fewer
    finite logits than k (5 of them, none where only k = 1 exists), 6 and 7 plain."""
    kmax = topk_kmax(V)
    rs = np.random.RandomState(V)
    pad, eos, unk = V - 1, max(V - 2, 0), min(5, max(V - 3, 0))
    x = (np.round(rs.randn(total, V) * 3 * 4) / 4).astype(np.float32)
    cum = -(rs.randint(0, 64, size=total) / 8).astype(np.float32)
    forced = np.full(total, -1, dtype=np.int64)
    for r in range(total):
        kind = r % SPECIALS
        if kind == 0:
            pairs = [(a, a + 1) for a in (255, 2047) if a + 2 < V] or [(0, max(V - 3, 0))]
            for a, b in pairs:
                x[r, a] = x[r, b] = 12.0
        elif kind == 1:
            x[r, rs.randint(0, V)] = np.nan
        elif kind == 2:
            forced[r] = rs.randint(0, max(V - 2, 1))
        elif kind == 3:
            forced[r] = pad
        elif kind == 4:
            cum[r] = -np.inf
        elif kind == 5:
            keep = rs.permutation(V)[: min(5, kmax // 2)]
            row = np.full(V, -np.inf, dtype=np.float32)
            row[keep] = x[r, keep]
            x[r] = row
    return x, cum, forced, pad, eos, unk


def topk_reference(x, cum, forced, pad, eos, unk, T, flags, dtype, n):
    """The scoring rules of one step (beam_ref.py:58-79) in `dtype`, then each row's top n."""
    with np.errstate(invalid="ignore"):
        lp = beam_ref.log_softmax(x.astype(dtype) / dtype(T), dtype)
    lp[lp != lp] = -np.inf
    lp[:, pad] = -np.inf
    lp[:, unk] -= dtype(UNK_PENALTY)
    if flags & 1:
        lp[:, :eos] = -np.inf
        lp[:, eos + 1:] = -np.inf
    for r in np.nonzero((forced >= 0) & (forced != pad))[0]:
        keep = lp[r, forced[r]]
        lp[r] = -np.inf
        lp[r, forced[r]] = keep
    if flags & 2:
        lp[(forced < 0) | (forced == pad), eos] = -np.inf
    return beam_ref.topk_lowest_index(lp + cum.astype(dtype)[:, None], n)
