"""The restatement of the diverse beam searches (tests/diverse_ref.py) against itself where the rules say so: lists
of 2*beam entries suffice (brute force over the whole vocabulary), one group is the beam step, strength 0 is a beam
search per group, rate 0 is the beam step; the decidability of the searches the GPU tests restate; and the host-side
surface (`DiverseBeamSearch`, `DiverseSiblingsSearch`, `SeqGenCustom`, `cfg.gen`).  No GPU."""
import numpy as np
import pytest
import torch

import beam_step_ref
import diverse_cases as DC
import diverse_ref as DR


def _scores(rs, beam, V, ties=True):
    """fp32 `lp + cum` [beam, V] with planted duplicates (inside a row and across rows) and a few -inf."""
    x = (np.log(rs.rand(beam, V)) - rs.rand(beam, 1) * 2).astype(np.float32)
    if ties:
        for _ in range(3 * beam):
            b0, b1 = rs.randint(0, beam, 2)
            x[b1, rs.randint(0, V)] = x[b0, rs.randint(0, V)]
        x[:, 3] = x[0, 3]  # one token, the same value in every row
        srt = np.sort(x, axis=1)
        for b in range(beam // 2):  # ties near the top, where the cut falls, between beams b and b + 2
            x[b, 7] = x[b + 2, 5] = srt[b, -2]
            x[b, 11] = x[b + 2, 12] = srt[b, -4]
    x[rs.rand(beam, V) < 0.1] = -np.inf
    return x


@pytest.mark.parametrize("lam", [0.5, 3.0])
@pytest.mark.parametrize("G", [2, 4])
def test_lists_of_2beam_entries_suffice(G, lam):
    beam, V, k = 4, 23, 8
    rs = np.random.RandomState(100 * G + int(lam * 10))
    hit = ties = 0
    for trial in range(60):
        x = _scores(rs, beam, V)
        rv, ri = beam_step_ref.row_lists(x, None, k)
        for step in (0, 3):
            cnt = DR.new_counters()
            got = DR.group_candidates(rv, ri, step, V, G, lam, cnt)
            want = DR.group_candidates_full(x, step, G, lam)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (trial, step)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (trial, step)
            hit += cnt["penalty_reordered"] > 0
            ties += cnt["cross_beam_tie"]
    # the penalty moved a group's choice, and ties between two beams of a group were broken by the index (G = 4 at
    # beam 4 has one beam per group: its ties are inside a row, between tokens)
    assert hit > 30 and (ties > 10 or G == beam)


def _lists_state(rs, bsz, beam, V, max_len, step, eos):
    st = beam_step_ref.new_state(bsz, beam, max_len, V - 1, eos, anc_ld=max_len + 2)
    st["tok"][:, 1: step + 1] = rs.randint(0, V - 2, (bsz * beam, step))
    st["sc"][:, :step] = -np.cumsum(rs.rand(bsz * beam, step), axis=1).astype(np.float32)
    x = np.stack([_scores(rs, beam, V) for _ in range(bsz)]).reshape(bsz * beam, V)
    x[:, V - 1] = -np.inf
    return st, beam_step_ref.row_lists(x, None, 2 * beam)


def _same_state(a, b):
    for key in a[0]:
        if a[0][key] is None:
            assert b[0][key] is None
            continue
        x, y = a[0][key], b[0][key]
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), key
    assert np.array_equal(a[1], b[1])


@pytest.mark.parametrize("step", [0, 1, 4])
def test_one_group_is_the_beam_step_and_rate_0_is_it_from_step_1_on(step):
    bsz, beam, V, max_len, eos = 3, 4, 23, 8, 21
    rs = np.random.RandomState(step)
    st, (rv, ri) = _lists_state(rs, bsz, beam, V, max_len, step, eos)
    want = beam_step_ref.step(st, rv, ri, step, V, eos, max_len)
    _same_state(DR.group_step(st, rv, ri, step, V, eos, max_len, 1, 0.5), want)
    _same_state(DR.group_step(st, rv, ri, step, V, eos, max_len, 1, 0.0), want)
    _same_state(DR.sibling_step(st, rv, ri, step, V, eos, max_len, 0.0), want)
    if step == 0:  # rule B: step 0 is the plain beam step at any rate
        _same_state(DR.sibling_step(st, rv, ri, step, V, eos, max_len, 0.7), want)
    else:
        c = DR.sibling_candidates(rv[:beam], ri[:beam], step, V, 0.7)
        plain = DR.sibling_candidates(rv[:beam], ri[:beam], step, V, 0.0)
        assert not np.array_equal(c[0], plain[0])


@pytest.mark.parametrize("step", [0, 2])
def test_strength_0_is_a_beam_search_per_group(step):
    beam, V, G = 4, 23, 2
    rs = np.random.RandomState(7 + step)
    x = _scores(rs, beam, V)
    rv, ri = beam_step_ref.row_lists(x, None, 2 * beam)
    sc, tok, bm = DR.group_candidates(rv, ri, step, V, G, 0.0)
    for g in range(G):
        beams = np.array([g]) if step == 0 else np.arange(g, beam, G)
        v, t, b = rv[beams].reshape(-1), ri[beams].reshape(-1), np.repeat(beams, 2 * beam)
        order = np.lexsort((b * V + t, -v.astype(np.float64)))[: 2 * beam // G]  # beam_step_ref.step's merge
        assert np.array_equal(sc[g::G].view(np.uint32), v[order].view(np.uint32))
        assert np.array_equal(tok[g::G], t[order]) and np.array_equal(bm[g::G], b[order])


def test_the_penalty_is_formed_in_fp32_and_counts_every_candidate():
    """One row per group, values chosen so that (v - lam * cnt) differs between fp32 and fp64 ranking."""
    beam, V, G = 2, 9, 2
    rv = np.array([[-1.0, -2, -3, -4], [-1.0, -1.25, -1.5, -8]], dtype=np.float32)
    ri = np.array([[5, 6, 7, 0], [5, 6, 0, 2]], dtype=np.int64)
    sc, tok, bm = DR.group_candidates(rv, ri, 1, V, G, 0.5)
    # group 0 took tokens 5, 6; group 1's entries 5 and 6 pay 0.5 each: -1.5, -1.75, token 0 stays at -1.5
    assert tok[1::2].tolist() == [0, 5] and sc[1::2].tolist() == [-1.5, -1.5] and bm.tolist() == [0, 1, 0, 1]
    lam = np.float32(0.1)
    sc, tok, bm = DR.group_candidates(rv, ri, 1, V, G, 0.1)
    assert sc[1] == np.float32(np.float32(-1.0) - lam) and sc[3] == np.float32(np.float32(-1.25) - lam)
    assert sc.dtype == np.float32


# ---- the searches the GPU tests restate are decidable ----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DC.STEP_CASES))
def test_the_scripted_step_searches_meet_what_they_plant(name):
    cnt, st = DC.run_scripted(name)[:2]
    assert st["remaining"][0] == 0
    for key in ("penalty_reordered", "cross_beam_tie", "neginf_candidate", "eos_inside_beam", "eos_beyond_beam",
                "ignored_beam", "idle_steps"):
        if key == "penalty_reordered" and DC.STEP_CASES[name].get("rate") is not None:
            continue  # rule B has no token penalty
        if key == "cross_beam_tie" and DC.STEP_CASES[name].get("groups") == DC.BEAM:
            continue  # one beam per group
        assert cnt[key] > 0, (name, key, cnt)


def test_min_gap_is_the_smallest_kept_rejected_distance():
    beam, V = 2, 9
    rv = np.array([[-1.0, -2, -3, -4], [-1.5, -2.5, -3.25, -8]], dtype=np.float32)
    ri = np.array([[5, 6, 7, 0], [5, 6, 0, 2]], dtype=np.int64)
    gaps = []
    DR.sibling_candidates(rv, ri, 1, V, 0.0, gaps=gaps)  # kept -1 -1.5 -2 -2.5 | -3
    assert gaps == [0.5] and DR.min_gap(gaps) == 0.5 and DR.min_gap([]) == np.inf
    gaps = []
    DR.group_candidates(rv, ri, 1, V, 2, 0.0, gaps=gaps)  # one row per group, two kept of four
    assert gaps == [1.0, 0.75]


# ---- the host-side surface -------------------------------------------------------------------------------------------
class _Tok:
    def __init__(self, n=40):
        self.n = n

    def __len__(self):
        return self.n

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


def test_refusals():
    from vidsitu_amd.seq_gen import DiverseBeamSearch, DiverseSiblingsSearch, Sampling, SeqGenCustom

    with pytest.raises(ValueError):
        SeqGenCustom([_LM()], _Tok(), beam_size=4, diverse_beam_groups=3)  # beam % G
    with pytest.raises(ValueError):
        SeqGenCustom([_LM()], _Tok(), beam_size=4, search_strategy=DiverseBeamSearch(_Tok(), 3, 0.5))
    with pytest.raises(ValueError):
        DiverseBeamSearch(_Tok(), 2, -0.5)
    with pytest.raises(ValueError):
        DiverseBeamSearch(_Tok(), 0, 0.5)
    with pytest.raises(ValueError):
        DiverseSiblingsSearch(_Tok(), -0.5)
    with pytest.raises(ValueError):
        SeqGenCustom([_LM()], _Tok(), beam_size=4, diverse_beam_groups=2, diverse_beam_strength=-1.0)
    with pytest.raises(ValueError):
        SeqGenCustom([_LM()], _Tok(), beam_size=4, diversity_rate=-0.5)
    for kw in (dict(diverse_beam_groups=2), dict(diversity_rate=0.5)):  # V - 1 = 8 < 2 * 4 + 1
        with pytest.raises(ValueError):
            SeqGenCustom([_LM()], _Tok(8), beam_size=4, **kw)
        assert SeqGenCustom([_LM()], _Tok(9), beam_size=4, **kw).search is not None
    for kw in (dict(sampling=True, diverse_beam_groups=2), dict(sampling=True, diversity_rate=0.5),
               dict(diverse_beam_groups=2, diversity_rate=0.5),
               dict(search_strategy=Sampling(_Tok()), diverse_beam_groups=2),
               dict(search_strategy=DiverseBeamSearch(_Tok(), 2), diversity_rate=0.5),
               dict(search_strategy=DiverseSiblingsSearch(_Tok(), 0.5), sampling=True)):
        with pytest.raises(ValueError):
            SeqGenCustom([_LM()], _Tok(), beam_size=4, **kw)
    with pytest.raises(NotImplementedError):
        SeqGenCustom([_LM()], _Tok(), search_strategy=object())
    for args in (dict(G=3), dict(G=2, lam=-0.5), dict(rate=-1.0)):
        with pytest.raises(ValueError):
            DR.check_args(4, 40, **args)
    with pytest.raises(ValueError):
        DR.check_args(4, 8, G=2)


def test_strategy_keys_tell_strategies_and_numbers_apart():
    from vidsitu_amd.seq_gen import DiverseBeamSearch, DiverseSiblingsSearch, SeqGenCustom

    def key(**kw):
        return SeqGenCustom([_LM()], _Tok(), beam_size=4, **kw)._strategy_key()

    keys = [key(), key(sampling=True), key(sampling=True, sampling_topk=2), key(diverse_beam_groups=2),
            key(diverse_beam_groups=4), key(diverse_beam_groups=2, diverse_beam_strength=2.0),
            key(diversity_rate=0.5), key(diversity_rate=2.0)]
    assert len(set(keys)) == len(keys) and keys[0] is None
    s = DiverseBeamSearch(_Tok(), num_groups=2, diversity_strength=0.5)
    gen = SeqGenCustom([_LM()], _Tok(), beam_size=4, search_strategy=s)
    assert gen.search is s and gen._strategy_key() == key(diverse_beam_groups=2)
    s = DiverseSiblingsSearch(_Tok(), diversity_rate=0.5)
    assert SeqGenCustom([_LM()], _Tok(), beam_size=4, search_strategy=s)._strategy_key() == key(diversity_rate=0.5)


def test_cfg_gen_keys_reach_the_generator():
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.seq_gen import DiverseBeamSearch, DiverseSiblingsSearch, SeqGenCustom

    cfg = get_cfg()
    assert (cfg.gen.diverse_beam_groups, cfg.gen.diverse_beam_strength, cfg.gen.diversity_rate) == (-1, 0.5, -1.0)
    assert SeqGenCustom([_LM()], _Tok(), **{k: cfg.gen[k] for k in cfg.gen}).search is None
    cfg = get_cfg({"gen.diverse_beam_groups": 2, "gen.beam_size": 4})
    gen = SeqGenCustom([_LM()], _Tok(), **{k: cfg.gen[k] for k in cfg.gen})  # as EvalB_Gen builds it
    assert isinstance(gen.search, DiverseBeamSearch)
    assert (gen.search.num_groups, gen.search.diversity_strength) == (2, 0.5)
    cfg = get_cfg({"gen.diversity_rate": 0.25, "gen.beam_size": 4})
    gen = SeqGenCustom([_LM()], _Tok(), **{k: cfg.gen[k] for k in cfg.gen})
    assert isinstance(gen.search, DiverseSiblingsSearch) and gen.search.diversity_rate == 0.25
    cfg = get_cfg({"gen.diverse_beam_groups": 2})  # beam_size 1 is no multiple of 2
    with pytest.raises(ValueError):
        SeqGenCustom([_LM()], _Tok(), **{k: cfg.gen[k] for k in cfg.gen})
