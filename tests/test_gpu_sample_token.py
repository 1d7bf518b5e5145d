"""`vs_sample_token` (plain / top-k / nucleus draws of one search step) against the fp64 restatement of
tests/sample_ref.py, on the inputs of tests/sample_cases.py: one block per row (V = 97), the first sliced V (2049), a V
that is no multiple of 4 (4099) and the real vocabulary's 25 slices (50261).

Acceptance of a draw (docs/beam_search_parity.md, "Sampling"): the kernel's token t lies in the reference's kept set
and u * S lies in [F(t-) - delta * S, F(t) + delta * S] of the reference's CDF over the kept set in ascending token id;
the value equals lp_t + cum to 1e-6 relative.  DEPARTURE from the issue, which says "1e-6 relative" of lp_t + cum:
this test takes 1e-6 of the largest fp32 term the value is formed from -- x_t / T, the row's log-sum-exp, cum -- each
of which is rounded at its own magnitude.  A likely token has x_t / T ~ lse ~ 20 and lp_t ~ -0.5, and cum may cancel
lp_t, so no fp32 evaluation (vs_beam_topk's included) holds 1e-6 of the result itself; seen on the GPU: 4.0e-7 absolute
on a value of 0.0385 (V = 97, row 4, x_t / T = 24).  The sharper pin beside it: on the top-k 1 and top-p 1e-6 rows of
the sliced vocabularies the value equals vs_beam_topk(k = 1)'s bit for bit.
delta = 1e-5 is derived there, not measured.  At V = 97 the token also
equals the fp64 inverse CDF, except for draws within delta of a CDF boundary, which are counted against a 2 % cap."""
import numpy as np
import pytest
import torch

import dropout_ref
import sample_cases as SC
import sample_ref as SR

pytestmark = pytest.mark.gpu
DELTA = SR.DELTA


def _state(dev, seed=SC.SEED, step=0):
    return torch.tensor([seed, step], dtype=torch.long, device=dev)


def _call(ops, c, variant, topk, topp, snap, dev, row_ids=None, one_block=False):
    v = c[variant]
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    val, idx = ops.sample_token(t(c["x"]), t(c["cum"]), t(v["forced"]), snap, c["pad"], c["eos"], c["unk"],
                                sampling_topk=topk, sampling_topp=topp, unk_penalty=SC.UNK_PENALTY,
                                temperature=SC.TEMPERATURE, eos_only=bool(v["flags"] & 1), ban_eos=bool(v["flags"] & 2),
                                tokens=t(v["tokens"]), step=SC.STEP,
                                no_repeat_ngram_size=SC.NGRAM if v["tokens"] is not None else 0,
                                row_ids=t(row_ids), one_block=one_block)
    return val.cpu().numpy(), idx.cpu().numpy()


def _accept(c, variant, topk, topp, u, val, idx):
    """Asserts the acceptance rule for every row, and that a token other than the fp64 inverse CDF's comes from a draw
    within delta of a CDF boundary; returns the number of such draws."""
    lp = c[variant]["lp"]
    near = 0
    xs = c["x"].astype(np.float64) / SC.TEMPERATURE
    lse = xs.max(1) + np.log(np.exp(xs - xs.max(1, keepdims=True)).sum(1))
    for r in range(c["rows"]):
        keep = SR.kept_set(lp[r], topk, topp)
        lo, hi, s = SR.cdf(lp[r], keep)
        t = int(idx[r])
        if s == 0.0:
            assert t == 0 and val[r] == -np.inf, (variant, r, t, val[r])
            continue
        pos = u[r] * s
        print(f"{variant} row {r}: token {t} u*S {pos:.9g} in [{lo[t]:.9g}, {hi[t]:.9g}] S {s:.9g}")
        assert keep[t], f"{variant} row {r}: token {t} is not in the reference's kept set"
        assert lo[t] - DELTA * s <= pos <= hi[t] + DELTA * s, (variant, r, t, pos, lo[t], hi[t], s)
        ref = float(lp[r, t]) + float(c["cum"][r])
        scale = max(abs(xs[r, t]), abs(lse[r]), abs(float(c["cum"][r])), abs(ref))
        assert abs(float(val[r]) - ref) <= 1e-6 * scale, (variant, r, float(val[r]), ref, scale)
        edges = np.concatenate([lo[keep], hi[keep][-1:]])
        at_edge = bool(np.min(np.abs(edges - pos)) <= DELTA * s)
        near += at_edge
        assert at_edge or t == SR.draw_row(lp[r], keep, u[r])[1], (variant, r, t, "away from every CDF boundary")
    return near


@pytest.mark.parametrize("mode", range(len(SC.MODE_NAMES)), ids=SC.MODE_NAMES)
@pytest.mark.parametrize("V", sorted(SC.SHAPES))
def test_draw_lies_in_the_reference_cdf(V, mode, dev):
    from vidsitu_amd import ops

    c = SC.case(V)
    _, topk, topp = SC.modes(V)[mode]
    state = _state(dev)
    for variant in SC.VARIANTS:
        snap = ops.dropout_tick(state)
        seed, step = (int(a) for a in snap.cpu())
        u = SR.uniforms(seed, step, np.arange(c["rows"]))
        val, idx = _call(ops, c, variant, topk, topp, snap, dev)
        _accept(c, variant, topk, topp, u, val, idx)
        # the same snapshot draws the same tokens, bit for bit, and so does the form with one block per row
        val2, idx2 = _call(ops, c, variant, topk, topp, snap, dev)
        assert np.array_equal(idx, idx2) and np.array_equal(val.view(np.uint32), val2.view(np.uint32))
        val3, idx3 = _call(ops, c, variant, topk, topp, snap, dev, one_block=True)
        assert np.array_equal(idx, idx3) and np.array_equal(val.view(np.uint32), val3.view(np.uint32))
        if topk == 1 or topp == 1e-6:  # one kept token: the arg-max of the scoring kernel
            v = c[variant]
            t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
            bv, bi = ops.beam_topk(t(c["x"]), t(c["cum"]), t(v["forced"]), 1, c["pad"], c["eos"], c["unk"],
                                   SC.UNK_PENALTY, SC.TEMPERATURE, eos_only=bool(v["flags"] & 1),
                                   ban_eos=bool(v["flags"] & 2), tokens=t(v["tokens"]), step=SC.STEP,
                                   no_repeat_ngram_size=SC.NGRAM if v["tokens"] is not None else 0)
            assert np.array_equal(bi.cpu().numpy()[:, 0], idx)
            if V > 2048:  # both kernels form the row's lse from the same slice partials: the value's bits are equal
                # (at V = 97 the scoring kernel sums the row in another order, so only the token is comparable)
                assert np.array_equal(bv.cpu().numpy()[:, 0].view(np.uint32), val.view(np.uint32))
    assert [int(a) for a in state.cpu()] == [SC.SEED, len(SC.VARIANTS)]  # one tick per draw, the seed untouched


def test_small_vocabulary_equals_the_fp64_inverse_cdf(dev):
    """V = 97, every mode, both variants, four ticks: the token is the fp64 inverse CDF's unless u * S lies within
    delta of a boundary; those draws are counted and capped at 2 % of all."""
    from vidsitu_amd import ops

    V = 97
    c = SC.case(V)
    state = _state(dev, step=7)
    total = near_total = 0
    for tick in range(4):
        snap = ops.dropout_tick(state)
        u = SR.uniforms(SC.SEED, 7 + tick, np.arange(c["rows"]))
        for _, topk, topp in SC.modes(V):
            for variant in SC.VARIANTS:
                val, idx = _call(ops, c, variant, topk, topp, snap, dev)
                near_total += _accept(c, variant, topk, topp, u, val, idx)
                total += c["rows"]
    print(f"{near_total} of {total} draws within delta of a CDF boundary")
    assert near_total <= 0.02 * total


@pytest.mark.parametrize("mode", ["plain", "topk40", "topp0.9"])
def test_sliced_form_replayed_from_a_graph_equals_eager(mode, dev):
    """The tick and the launches of the sliced form captured once and replayed three times: every replay draws with
    the next step's words and gives the bits of an eager call on the same snapshot (what a captured search step
    does from its third use on; everything between the launches must be re-made by the launches themselves)."""
    from vidsitu_amd import ops

    V = 4099
    c = SC.case(V)
    _, topk, topp = SC.modes(V)[SC.MODE_NAMES.index(mode)]
    v = c["ban"]
    x, cum, forced, tokens = (torch.from_numpy(a).to(dev) for a in (c["x"], c["cum"], v["forced"], v["tokens"]))
    kw = dict(sampling_topk=topk, sampling_topp=topp, unk_penalty=SC.UNK_PENALTY, temperature=SC.TEMPERATURE,
              ban_eos=True, tokens=tokens, step=SC.STEP, no_repeat_ngram_size=SC.NGRAM)
    state, snap = _state(dev, step=20), torch.zeros(2, dtype=torch.long, device=dev)
    ops.sample_token(x, cum, forced, _state(dev), c["pad"], c["eos"], c["unk"], **kw)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.dropout_tick(state, out=snap)
        val, idx = ops.sample_token(x, cum, forced, snap, c["pad"], c["eos"], c["unk"], **kw)
    drawn = []
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert snap.tolist() == [SC.SEED, 20 + i]
        got = (val.cpu().numpy().copy(), idx.cpu().numpy().copy())
        want = ops.sample_token(x, cum, forced, snap.clone(), c["pad"], c["eos"], c["unk"], **kw)
        assert np.array_equal(got[1], want[1].cpu().numpy()), (i, got[1], want[1])
        assert np.array_equal(got[0].view(np.uint32), want[0].cpu().numpy().view(np.uint32)), i
        _accept(c, "ban", topk, topp, SR.uniforms(SC.SEED, 20 + i, np.arange(c["rows"])), *got)
        drawn.append(got[1])
    assert not (np.array_equal(drawn[0], drawn[1]) and np.array_equal(drawn[1], drawn[2]))


def test_row_ids_and_ticks_select_the_generator_words(dev):
    """A row draws with the word of row_ids[r] (the host search's shrunken batch), and the next tick's snapshot draws
    from the next step's words of tests/dropout_ref.words."""
    from vidsitu_amd import ops

    V = 2049
    c = SC.case(V)
    state = _state(dev, step=3)
    ids = np.array([40, 3, 17, 5, 1000003, 2 ** 33 + 1], dtype=np.int64)
    drawn = []
    for tick in range(2):
        snap = ops.dropout_tick(state)
        assert [int(a) for a in snap.cpu()] == [SC.SEED, 3 + tick]
        w = dropout_ref.words(SC.SEED, 3 + tick, SR.SAMPLE_SITE, ids.astype(np.uint64))
        u = (w.astype(np.float64) + 0.5) / 2.0 ** 32
        val, idx = _call(ops, c, "ban", -1, -1.0, snap, dev, row_ids=ids)
        _accept(c, "ban", -1, -1.0, u, val, idx)
        drawn.append(idx)
    assert not np.array_equal(drawn[0], drawn[1])


def test_refusals(dev):
    from vidsitu_amd import _lib, ops

    c = SC.case(97)
    with pytest.raises(_lib.VsError):
        _call(ops, c, "last", 5, 0.5, _state(dev), dev)
    with pytest.raises(_lib.VsError):
        _call(ops, c, "last", -1, 1.5, _state(dev), dev)
