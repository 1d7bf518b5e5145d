"""CPU checks behind the beam-search GPU tests (no GPU): the step-level restatement
(tests/beam_step_ref.py) chained into a whole search returns the oracle's hypotheses, bit for bit; the
scripted lists of tests/test_gpu_beam_step.py reach every branch they are meant to reach; and the
conditions that make token / index equality decidable on the GPU hold for every case, from the
reference alone (fp32 against fp64 numpy)."""
import numpy as np
import pytest

import beam_cases as C
import beam_step_ref as S
from oracle import beam_ref


def _assert_bitwise(got, want, what):
    assert len(got) == len(want)
    for sg, sw in zip(got, want):
        assert len(sg) == len(sw), what
        for hg, hw in zip(sg, sw):
            assert hg["tokens"].tolist() == hw["tokens"].tolist(), what
            assert np.float32(hg["score"]).tobytes() == np.float32(hw["score"]).tobytes(), what
            assert hg["positional_scores"].astype(np.float32).tobytes() == \
                hw["positional_scores"].astype(np.float32).tobytes(), what


@pytest.mark.parametrize("name", list(C.SEARCH_CASES))
def test_chained_step_returns_the_oracles_hypotheses(name):
    a, b, w, prefix, kw = C.search_inputs(C.SEARCH_CASES[name])
    got = S.search(C.hash_step_logits(a, b, w), **kw)
    _assert_bitwise(got, C.search_oracle(name), name)


@pytest.mark.parametrize("V,beam", [(3, 2), (4, 3), (5, 4), (6, 3), (6, 5), (7, 5), (8, 4), (12, 5)])
def test_chained_step_equals_the_oracle_at_small_vocabularies(V, beam):
    """History-dependent logits on a 0.25 grid (designed ties), min_len 0..2, with and without a penalty."""
    counters = S.new_counters()
    for seed in range(12):
        rs = np.random.RandomState(seed * 31 + V)
        a = (np.round(rs.randn(C.HASH_A, V) * 4) / 4).astype(np.float32)
        b = (np.round(rs.randn(C.HASH_B, V) * 4) / 4).astype(np.float32)
        eos = seed % (V - 1)  # any token but pad = V - 1
        kw = dict(bsz=3, vocab=V, pad=V - 1, eos=eos, unk=(eos + 1) % (V - 1), beam_size=beam, max_len_b=7,
                  min_len=seed % 3, unk_penalty=0.25 * (seed % 2), len_penalty=(1.0, 0.5, 2.0)[seed % 3],
                  normalize_scores=seed % 4 != 3)
        f = C.hash_step_logits(a, b, C.hash_weights(9))
        _assert_bitwise(S.search(f, counters=counters, **kw), beam_ref.generate(f, **kw), f"seed {seed}")
    if V <= beam + 1:  # fewer live tokens than beams: ignored candidates must fill up
        assert counters["ignore_set"] > 0, counters


def test_scripted_lists_reach_every_branch():
    """The restatement's counters over the step-level case list: an edited generator cannot silently stop
    reaching a branch.  Per case, what it is there for."""
    total = S.new_counters()
    per = {}
    for name, case in C.STEP_CASES.items():
        cnt = S.new_counters()
        idle = np.zeros(case["bsz"], dtype=np.int64)  # steps a finished sentence sat through while others ran

        def on_step(step, row_val, row_idx, st, reorder, idle=idle):
            idle += (st["finished"] != 0) & (st["remaining"][0] > 0)
        C.run_step_case(case, cnt, on_step)
        per[name] = cnt
        cnt["longest_idle"] = int(idle.max())
        for key in total:
            total[key] += cnt[key]
    print({k: int(v) for k, v in total.items()})
    assert all(total[key] > 0 for key in S.COUNTERS), total
    for name, case in C.STEP_CASES.items():
        assert all(per[name][key] > 0 for key in case["expect"]), (name, per[name])
    for name in C.LONG_IDLE:
        assert per[name]["longest_idle"] >= 10, (name, per[name])


def test_scripted_lists_are_exact_in_fp32():
    """Every list value is a multiple of 2^-6 below 2^11 (or -inf): fp32 holds it exactly, so kernel and
    restatement see identical numbers and nothing in the step-level comparison needs a tolerance."""
    def check(step, row_val, row_idx, st, reorder):
        fin = row_val[np.isfinite(row_val)].astype(np.float64)
        assert np.all(fin % C.GRID == 0) and np.all(np.abs(fin) < 2 ** 11)
        assert not np.isnan(row_val).any() and not np.isposinf(row_val).any()
    for case in C.STEP_CASES.values():
        C.run_step_case(case, on_step=check)


@pytest.mark.parametrize("V", C.TOPK_V + sorted({v for v, _ in C.TOPK_BIG}))
def test_topk_inputs_make_index_equality_decidable(V):
    """Part 3's condition: in fp64, any two entries among a row's top k + 1 that come from different
    logits differ by >= 1e-3 (equal logits give bit-equal scores on either side)."""
    kmax = C.topk_kmax(V)
    for total in ({160, C.SPECIALS} if V in C.TOPK_V else {C.SPECIALS}):
        x, cum, forced, pad, eos, unk = C.topk_inputs(V, total)
        for T in C.TOPK_T:
            for flags in (0, 1, 2):
                n = min(kmax + 1, V)
                v, i = C.topk_reference(x, cum, forced, pad, eos, unk, T, flags, np.float64, n)
                gap = v[:, :-1] - v[:, 1:]
                same_logit = np.take_along_axis(x, i[:, :-1], 1) == np.take_along_axis(x, i[:, 1:], 1)
                same_logit &= (i[:, :-1] != unk) & (i[:, 1:] != unk)
                close = np.isfinite(gap) & (gap < 1e-3) & ~same_logit
                assert not close.any(), (V, total, T, flags, gap[close])
                assert np.all(gap[np.isfinite(gap) & same_logit] == 0)


@pytest.mark.parametrize("name", list(C.SEARCH_CASES))
def test_search_cases_are_decidable_in_fp32(name):
    """Part 4's conditions: the oracle returns the same tokens in fp32 and in fp64, and in the fp64 run
    the smallest non-zero gap between adjacent entries of the top k + 1 flattened scores is >= 1e-4 at
    every step (1e-4 is the search tests' score tolerance; fp32 noise on |score| <= 100 is ~1e-5)."""
    a, b, w, prefix, kw = C.search_inputs(C.SEARCH_CASES[name])
    f = C.hash_step_logits(a, b, w)
    trace = []
    want64 = beam_ref.generate(f, dtype=np.float64, trace=trace, **kw)
    want32 = C.search_oracle(name)
    assert [[h["tokens"].tolist() for h in s] for s in want32] == [[h["tokens"].tolist() for h in s] for s in want64]
    gaps = np.concatenate([(t[:, :-1] - t[:, 1:]).ravel() for t in trace])
    gaps = gaps[np.isfinite(gaps) & (gaps != 0)]
    print(f"{name}: {len(trace)} steps, smallest non-zero gap {gaps.min():.3e}")
    assert gaps.min() >= 1e-4
    for s64, s32 in zip(want64, want32):
        for h64, h32 in zip(s64, s32):
            assert abs(h64["score"] - h32["score"]) < 2e-5


def test_beam_sizes_above_16_are_refused():
    """2*beam entries per row exceed the scoring kernel's 32-entry lists: refused at construction, not at
    the first step of a search."""
    import torch

    from vidsitu_amd.seq_gen import SeqGenCustom

    class Tok:
        def __len__(self):
            return 100

        def pad(self):
            return 1

        def eos(self):
            return 2

        def unk(self):
            return 3

    class LM(torch.nn.Module):
        use_encoder = False

    for device_search in (True, False):
        with pytest.raises(NotImplementedError, match="32"):
            SeqGenCustom([LM()], Tok(), beam_size=17, device_search=device_search)
        assert SeqGenCustom([LM()], Tok(), beam_size=16, device_search=device_search).beam_size == 16
