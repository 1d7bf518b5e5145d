"""CPU anchors of the sampling tests: the restatement (tests/sample_ref.py) against the oracle's beam search where the
two must agree, the properties the committed fixtures (tests/sample_cases.py) need for the kernel test's acceptance
rule to be decidable, and the host-side surface (`Sampling`, `SeqGenCustom`, `cfg.gen`)."""
import numpy as np
import pytest
import torch

import beam_ngram_ref
import sample_cases as SC
import sample_ref as SR
from oracle import beam_ref

DELTA = SR.DELTA


@pytest.mark.parametrize("V,seed", [(12, 2), (40, 4)])
def test_topk_1_with_one_beam_is_the_oracles_greedy_search(V, seed):
    table, hist, prefix = beam_ngram_ref.stub_tables(V, seed, 2)
    step_logits = beam_ngram_ref.stub_step_logits(table, hist)
    kw = dict(bsz=2, vocab=V, pad=1, eos=2, unk=3, beam_size=1, max_len_b=16, min_len=3, prefix_tokens=prefix)
    want = beam_ref.generate(step_logits, **kw)
    got, _ = SR.search(step_logits, seed=9, sampling_topk=1, **kw)
    assert [[h["tokens"].tolist() for h in s] for s in got] == [[h["tokens"].tolist() for h in s] for s in want]
    for hg, hw in zip(sum(got, []), sum(want, [])):
        assert abs(hg["score"] - hw["score"]) <= 1e-5 * abs(hw["score"])
        assert np.allclose(hg["positional_scores"], hw["positional_scores"], atol=1e-5)


def test_sampling_search_draws_with_replacement_and_finishes_every_beam():
    """Plain sampling on the stub decoder: every sentence ends with `beam` hypotheses, step 0 draws per beam (two
    beams of a sentence may start with the same token), another seed gives other captions."""
    V = 40
    table, hist, _ = beam_ngram_ref.stub_tables(V, 4, 3)
    step_logits = beam_ngram_ref.stub_step_logits(table, hist)
    kw = dict(bsz=3, vocab=V, pad=1, eos=2, unk=3, beam_size=4, max_len_b=10, min_len=2, no_repeat_ngram_size=2)
    a, _ = SR.search(step_logits, seed=1, **kw)
    b, _ = SR.search(step_logits, seed=2, **kw)
    assert all(len(s) == 4 for s in a + b)
    toks = lambda fin: [[h["tokens"].tolist() for h in s] for s in fin]
    assert toks(a) != toks(b)
    assert not any(beam_ngram_ref.has_repeated_ngram([2] + h, 2) for s in toks(a) for h in s)


@pytest.mark.parametrize("V", sorted(SC.SHAPES))
def test_fixtures_have_no_nucleus_boundary_within_delta(V):
    """Token i + 1 of the ranking is kept iff the cumulative mass of the first i is < topp.  The kernel's sums carry a
    relative error (below delta: the parity document), so the comparison of a sum c with topp can only turn where
    |c - topp| <= delta * max(c, topp): no sum of the fixtures lies there.  A row without mass has no kept set to get
    wrong (it returns (-inf, 0))."""
    c = SC.case(V)
    for variant in SC.VARIANTS:
        lp = c[variant]["lp"]
        for name, _, topp in SC.modes(V):
            if topp <= 0:
                continue
            for r in range(c["rows"]):
                cum = np.cumsum(np.exp(lp[r])[SR.ranked(lp[r])])[:-1]
                if cum[-1] == 0.0:
                    continue
                gap = float(np.min(np.abs(cum - topp) / np.maximum(cum, topp)))
                assert gap > DELTA, (V, variant, name, r, gap)


@pytest.mark.parametrize("V", sorted(SC.SHAPES))
def test_fixtures_have_no_tied_topk_boundary(V):
    c = SC.case(V)
    for variant in SC.VARIANTS:
        lp = c[variant]["lp"]
        for name, topk, _ in SC.modes(V):
            if topk <= 0 or topk >= V:
                continue
            for r in range(c["rows"]):
                order = SR.ranked(lp[r])
                last_in, first_out = lp[r][order[topk - 1]], lp[r][order[topk]]
                assert last_in > first_out or last_in == -np.inf, (V, variant, name, r)  # -inf ties carry no mass


def test_fixtures_draw_rarely_within_delta_of_a_cdf_boundary():
    """V = 97, the ticks of test_gpu_sample_token.py: at most 2 % of the draws land within delta of a boundary."""
    V = 97
    c = SC.case(V)
    total = near = 0
    for step in list(range(7, 11)) + [0, 1]:
        u = SR.uniforms(SC.SEED, step, np.arange(c["rows"]))
        for _, topk, topp in SC.modes(V):
            for variant in SC.VARIANTS:
                lp = c[variant]["lp"]
                for r in range(c["rows"]):
                    keep = SR.kept_set(lp[r], topk, topp)
                    lo, hi, s = SR.cdf(lp[r], keep)
                    if s == 0.0:
                        continue
                    edges = np.concatenate([lo[keep], hi[keep][-1:]])
                    near += bool(np.min(np.abs(edges - u[r] * s)) <= DELTA * s)
                    total += 1
    assert total > 500 and near <= 0.02 * total, (near, total)


def test_fixtures_cover_an_all_banned_row_and_a_one_token_row():
    c = SC.case(97)
    assert np.isneginf(c["ban"]["lp"][2]).all()
    assert (np.isfinite(c["last"]["lp"]).sum(1) == 1).all()
    assert np.isneginf(c["ban"]["lp"][1, int(np.argmax(c["x"][1]))])


# ---- the host-side surface -----------------------------------------------------------------------------------------
class _Tok:
    def __len__(self):
        return 40

    def pad(self):
        return 1

    def eos(self):
        return 2

    def unk(self):
        return 3


class _LM(torch.nn.Module):
    use_encoder = False

    def __init__(self):
        super().__init__()
        self.decoder = torch.nn.Identity()


def test_constructor_refusals():
    from vidsitu_amd.seq_gen import Sampling, SeqGenCustom

    with pytest.raises(ValueError):
        Sampling(None, sampling_topk=5, sampling_topp=0.5)
    for topp in (0.0, 1.5, -0.5):
        with pytest.raises(ValueError):
            Sampling(None, sampling_topp=topp)
    with pytest.raises(ValueError):
        Sampling(None, sampling_topk=0)
    with pytest.raises(ValueError):
        SeqGenCustom([_LM()], _Tok(), sampling=True, sampling_topk=5, sampling_topp=0.5)
    with pytest.raises(ValueError):
        SeqGenCustom([_LM()], _Tok(), sampling_topk=5)  # a knob without sampling=True
    with pytest.raises(NotImplementedError):
        SeqGenCustom([_LM()], _Tok(), search_strategy=object())
    s = Sampling(_Tok(), sampling_topp=1.0)
    gen = SeqGenCustom([_LM()], _Tok(), search_strategy=s, beam_size=16)
    assert gen.search is s and gen._strategy_key() == (-1, 1.0)
    assert SeqGenCustom([_LM()], _Tok()).search is None
    with pytest.raises(NotImplementedError):
        SeqGenCustom([_LM()], _Tok(), sampling=True, beam_size=17)


def test_cfg_gen_keys_reach_the_generator():
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.seq_gen import SeqGenCustom

    cfg = get_cfg()
    assert (cfg.gen.sampling, cfg.gen.sampling_topk, cfg.gen.sampling_topp, cfg.gen.seed) == (False, -1, -1.0, 1)
    assert SeqGenCustom([_LM()], _Tok(), **{k: cfg.gen[k] for k in cfg.gen}).search is None
    cfg = get_cfg({"gen.sampling": True, "gen.sampling_topp": 0.9, "gen.seed": 3})
    gen = SeqGenCustom([_LM()], _Tok(), **{k: cfg.gen[k] for k in cfg.gen})  # as EvalB_Gen builds it
    assert gen.search.sampling_topp == 0.9 and gen.search.sampling_topk == -1 and gen.seed == 3
    cfg = get_cfg({"gen.sampling": True, "gen.sampling_topk": 40})
    assert SeqGenCustom([_LM()], _Tok(), **{k: cfg.gen[k] for k in cfg.gen}).search.sampling_topk == 40
