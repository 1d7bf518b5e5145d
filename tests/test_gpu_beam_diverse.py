"""The diverse beam searches of `vidsitu_amd.seq_gen` (`DiverseBeamSearch`, `DiverseSiblingsSearch`,
`gen.diverse_beam_groups` / `gen.diversity_rate`) on the GPU: the step's bookkeeping (`vs_beam_diverse_step`) against
the numpy steps of tests/diverse_ref.py bit for bit over the scripted search of tests/diverse_cases.py; one group
without strength == `vs_beam_step`; whole searches of the GPT-2 slice and the tiny fairseq-style decoder against
`diverse_ref.search` fed with the device's own per-step logits; host loop == device loop; eager / captured / replayed
steps; the options through the plugin surface and `main_dist.py`."""
import numpy as np
import pytest
import torch

import beam_ngram_ref
import beam_step_ref
import diverse_cases as DC
import diverse_ref as DR
from test_gpu_sample_search import _assert_same, _recorded, _setup, _toks

pytestmark = pytest.mark.gpu


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(_bits(got), _bits(want)), what


def _knobs(case):
    """(groups, strength, sibling_rate) of the C ABI."""
    if case.get("rate") is not None:
        return 0, 0.0, case["rate"]
    return case["groups"], case["lam"], 0.0


def _device_steps(dev, steps, start, step_fn):
    """Chain `step_fn` over the recorded steps [(step, state before, row_val, row_idx, want, want_reorder)] and hold
    every buffer to the restatement, bit for bit."""
    bsz, beam, max_len = DC.BSZ, DC.BEAM, DC.MAX_LEN
    rows = bsz * beam
    d = {key: torch.from_numpy(a.copy()).to(dev) for key, a in start.items()}
    tok = [d["tok"], torch.empty_like(d["tok"])]
    sc = [d["sc"], torch.empty_like(d["sc"])]
    anc = [d["anc"], torch.empty_like(d["anc"])]
    reorder = torch.empty(rows, dtype=torch.long, device=dev)
    for step, before, row_val, row_idx, want, want_reorder in steps:
        cur = step & 1
        d["ignore"].copy_(torch.from_numpy(before["ignore"]))  # the scripted search plants an ignored beam
        tok[1 - cur].fill_(-5)
        sc[1 - cur].fill_(77.0)
        anc[1 - cur].fill_(-9)
        reorder.fill_(-1)
        step_fn(torch.from_numpy(row_val).to(dev), torch.from_numpy(row_idx).to(dev), tok[cur], tok[1 - cur], sc[cur],
                sc[1 - cur], d["ignore"], d["finished"], d["nfin"], d["remaining"], d["fin_tok"], d["fin_score"],
                d["fin_pos"], d["fin_len"], reorder, step, anc[cur], anc[1 - cur])
        what = f"step {step}"
        _same(tok[1 - cur], want["tok"], what + " tok")
        _same(sc[1 - cur], want["sc"], what + " sc")
        for key in ("ignore", "finished", "nfin", "remaining", "fin_tok", "fin_score", "fin_pos", "fin_len"):
            _same(d[key], want[key], f"{what} {key}")
        _same(reorder, want_reorder, what + " reorder")
        got = anc[1 - cur].cpu().numpy()
        assert np.array_equal(got[:, : step + 2], want["anc"][:, : step + 2]), what + " anc"
        assert (got[:, step + 2:] == -9).all(), what + " anc: written past position step + 1"
    assert int(d["remaining"]) == 0


@pytest.mark.parametrize("name", sorted(DC.STEP_CASES))
def test_vs_beam_diverse_step_equals_the_restatement(name, dev):
    """bsz 5, beam 4, V 50, max_len 9; G = 2, G = 4 and siblings.  Planted and counted: one token on top of every
    row of a sentence (the penalty reorders the later groups), exact ties between two beams of a group (G = 4 has one
    beam per group at beam 4: no such tie exists there), -inf candidates, eos inside and beyond the first `beam`
    interleaved candidates, an ignored beam, a sentence that finishes at step 2 and idles."""
    from vidsitu_amd import ops

    case = DC.STEP_CASES[name]
    steps = []
    cnt, final, _ = DC.run_scripted(name, on_step=lambda *a: steps.append(a))
    for key in ("penalty_reordered", "cross_beam_tie", "neginf_candidate", "eos_inside_beam", "eos_beyond_beam",
                "ignored_beam", "idle_steps"):
        if (key == "penalty_reordered" and case.get("rate") is not None) or \
                (key == "cross_beam_tie" and case.get("groups") == DC.BEAM):
            continue
        assert cnt[key] > 0, (key, cnt)
    groups, strength, rate = _knobs(case)
    start = beam_step_ref.new_state(DC.BSZ, DC.BEAM, DC.MAX_LEN, DC.PAD, DC.EOS, anc_ld=DC.MAX_LEN + 2)

    def step_fn(rv, ri, tok_in, tok_out, sc_in, sc_out, ignore, finished, nfin, remaining, fin_tok, fin_score, fin_pos,
                fin_len, reorder, step, anc_in, anc_out):
        ops.beam_diverse_step(rv, ri, tok_in, tok_out, sc_in, sc_out, ignore, finished, nfin, remaining, fin_tok,
                              fin_score, fin_pos, fin_len, reorder, DC.BSZ, DC.BEAM, 2 * DC.BEAM, DC.V, step,
                              DC.MAX_LEN, DC.EOS, True, 1.0, groups, strength, rate, anc_in=anc_in, anc_out=anc_out)

    _device_steps(dev, steps, start, step_fn)


def test_one_group_without_strength_is_vs_beam_step(dev):
    """The same lists through `vs_beam_step` and through `vs_beam_diverse_step(groups=1, strength=0)`, chained over a
    whole scripted search: every output buffer bit for bit (and both equal to the restated beam step)."""
    from vidsitu_amd import ops

    steps = []
    DC.run_scripted(dict(groups=1, lam=0.0), on_step=lambda *a: steps.append(a))
    for step, before, rv, ri, want, want_reorder in steps:  # the restated diverse step with one group is the beam step
        ref, ref_reorder = beam_step_ref.step(before, rv, ri, step, DC.V, DC.EOS, DC.MAX_LEN)
        assert np.array_equal(ref_reorder, want_reorder)
        assert all(np.array_equal(_bits(ref[key]), _bits(want[key])) for key in ref)
    start = beam_step_ref.new_state(DC.BSZ, DC.BEAM, DC.MAX_LEN, DC.PAD, DC.EOS, anc_ld=DC.MAX_LEN + 2)

    def plain(rv, ri, tok_in, tok_out, sc_in, sc_out, ignore, finished, nfin, remaining, fin_tok, fin_score, fin_pos,
              fin_len, reorder, step, anc_in, anc_out):
        ops.beam_step(rv, ri, tok_in, tok_out, sc_in, sc_out, ignore, finished, nfin, remaining, fin_tok, fin_score,
                      fin_pos, fin_len, reorder, DC.BSZ, DC.BEAM, 2 * DC.BEAM, DC.V, step, DC.MAX_LEN, DC.EOS, True,
                      1.0, anc_in=anc_in, anc_out=anc_out)

    def diverse(rv, ri, tok_in, tok_out, sc_in, sc_out, ignore, finished, nfin, remaining, fin_tok, fin_score,
                fin_pos, fin_len, reorder, step, anc_in, anc_out):
        ops.beam_diverse_step(rv, ri, tok_in, tok_out, sc_in, sc_out, ignore, finished, nfin, remaining, fin_tok,
                              fin_score, fin_pos, fin_len, reorder, DC.BSZ, DC.BEAM, 2 * DC.BEAM, DC.V, step,
                              DC.MAX_LEN, DC.EOS, True, 1.0, 1, 0.0, 0.0, anc_in=anc_in, anc_out=anc_out)

    _device_steps(dev, steps, start, plain)
    _device_steps(dev, steps, start, diverse)


def test_vs_beam_diverse_step_refusals(dev):
    from vidsitu_amd import _lib, ops

    beam, V, max_len = 4, 50, 4
    st = beam_step_ref.new_state(1, beam, max_len, V - 1, V - 2)
    d = {key: torch.from_numpy(a).to(dev) for key, a in st.items() if a is not None}
    out = torch.empty(beam, dtype=torch.long, device=dev)
    rv, ri = torch.zeros(beam, 2 * beam, device=dev), torch.zeros(beam, 2 * beam, dtype=torch.long, device=dev)
    #            k         V   groups strength rate
    for bad in ((2 * beam, V, 3, 0.5, 0.0), (2 * beam - 1, V, 2, 0.5, 0.0), (2 * beam, 2 * beam, 2, 0.5, 0.0),
                (2 * beam, V, 2, -0.5, 0.0), (2 * beam, V, 0, 0.0, -0.5), (2 * beam, V, 2, 0.5, 0.5),
                (2 * beam, V, -1, 0.5, 0.0)):
        k, vocab, groups, strength, rate = bad
        with pytest.raises(_lib.VsError):
            ops.beam_diverse_step(rv, ri, d["tok"], d["tok"].clone(), d["sc"], d["sc"].clone(), d["ignore"],
                                  d["finished"], d["nfin"], d["remaining"], d["fin_tok"], d["fin_score"], d["fin_pos"],
                                  d["fin_len"], out, 1, beam, k, vocab, 0, max_len, V - 2, True, 1.0, groups, strength,
                                  rate)


# ---- whole searches --------------------------------------------------------------------------------------------------
def _reference(calls, tok, vocab, bsz, prefix, **kw):
    """`diverse_ref.search` on the device's own logits: the step callback refuses rows the device did not have."""
    def step_logits(tokens, sent_ids):
        t, logits = calls[tokens.shape[1] - 1]
        assert np.array_equal(t, tokens), f"the searches part before step {tokens.shape[1] - 1}"
        return logits

    return DR.search(step_logits, bsz, vocab, tok.pad(), tok.eos(), tok.unk(), prefix_tokens=prefix.cpu().numpy(), **kw)


def _gen_kw(knobs):
    kw = {k: v for k, v in knobs.items() if k == "no_repeat_ngram_size"}
    if "rate" in knobs:
        return dict(kw, diversity_rate=knobs["rate"])
    return dict(kw, diverse_beam_groups=knobs["groups"], diverse_beam_strength=knobs["strength"])


KNOBS = {"G2": dict(groups=2, strength=0.5), "G4": dict(groups=4, strength=0.5),
         "G2-ngram3": dict(groups=2, strength=0.5, no_repeat_ngram_size=3), "siblings": dict(rate=0.5)}


@pytest.mark.parametrize("knobs", list(KNOBS))
@pytest.mark.parametrize("name", ["gpt2", "txdec"])
def test_device_search_equals_the_restatement(name, knobs, dev):
    """Without a KV cache every step runs eagerly, so its logits can be recorded and fed to the restatement."""
    from vidsitu_amd.seq_gen import SeqGenCustom

    bsz, beam = 3, 4
    lm, tok, vocab, sample, prefix = _setup(name, dev, bsz)
    kw = dict(beam_size=beam, max_len_b=12, min_len=2)
    gen = SeqGenCustom([lm], tok, use_kv_cache=False, **kw, **_gen_kw(KNOBS[knobs]))
    calls = _recorded(gen)
    got = gen._generate(sample, prefix_tokens=prefix)
    gaps = []
    want = _reference(calls, tok, vocab, bsz, prefix, gaps=gaps, **kw, **KNOBS[knobs])
    print(f"{name} {knobs}: decidability gap {DR.min_gap(gaps):.3e} over {len(gaps)} merges")
    assert DR.min_gap(gaps) >= 1e-4
    _assert_same(got, want, 1e-5)
    assert all(len(s) == beam for s in got)
    if KNOBS[knobs].get("no_repeat_ngram_size"):
        assert not any(beam_ngram_ref.has_repeated_ngram([tok.eos()] + h, 3) for s in _toks(got) for h in s)


@pytest.mark.parametrize("name", ["gpt2", "txdec"])
def test_strong_groups_start_with_different_tokens_where_beam_search_repeats_one(name, dev):
    """What the feature is for, with G = 4 and strength 3.0 at beam 4 (one beam per group): in the restatement of the
    device's search, the four groups' first tokens after the prefix are pairwise different in every sentence; the
    plain beam search of the same decoder and prefixes ends with hypotheses that repeat a first token.  Two sentences:
    after the third prefix of `_setup` the GPT-2 slice puts one token more than 3.0 above every other, which no
    strength of 3.0 can move a group away from."""
    from vidsitu_amd.seq_gen import SeqGenCustom

    bsz, beam = 2, 4
    lm, tok, vocab, sample, prefix = _setup(name, dev, bsz)
    kw = dict(beam_size=beam, max_len_b=12, min_len=2)
    gen = SeqGenCustom([lm], tok, use_kv_cache=False, diverse_beam_groups=4, diverse_beam_strength=3.0, **kw)
    calls = _recorded(gen)
    got = gen._generate(sample, prefix_tokens=prefix)
    gaps, trace = [], []
    want = _reference(calls, tok, vocab, bsz, prefix, gaps=gaps, trace=trace, groups=4, strength=3.0, **kw)
    print(f"{name}: decidability gap {DR.min_gap(gaps):.3e}")
    assert DR.min_gap(gaps) >= 1e-4
    _assert_same(got, want, 1e-5)
    first = trace[1]["tok"][:, 2].reshape(bsz, beam)  # after step 1: [bos, prefix, first free token]
    plain = SeqGenCustom([lm], tok, use_kv_cache=False, **kw)._generate(sample, prefix_tokens=prefix)
    plain_first = [[h[1] for h in s] for s in _toks(plain)]
    print("groups' first tokens", first.tolist(), "beam search's", plain_first)
    assert all(len(set(row)) == beam for row in first.tolist())
    assert any(len(set(row)) < beam for row in plain_first)


@pytest.mark.parametrize("name,kv", [("gpt2", True), ("gpt2", False), ("txdec", True)])
@pytest.mark.parametrize("knobs", ["G2", "siblings"])
def test_host_search_equals_device_search(name, kv, knobs, dev):
    from vidsitu_amd.seq_gen import SeqGenCustom

    lm, tok, vocab, sample, prefix = _setup(name, dev, 3)
    outs = []
    for device_search in (True, False):
        gen = SeqGenCustom([lm], tok, beam_size=4, max_len_b=12, min_len=1, use_kv_cache=kv,
                           device_search=device_search, **_gen_kw(KNOBS[knobs]))
        outs.append(gen._generate(sample, prefix_tokens=prefix))
    # the host loop drops finished sentences from the batch, so its decoder runs at other row counts than the device
    # search's and rounds its logits otherwise: the search tolerance of test_gpu_gpt2.py (1e-4), tokens equal
    _assert_same(outs[1], outs[0], 1e-4)
    for hd, hh in zip(sum(outs[0], []), sum(outs[1], [])):
        assert np.allclose(hd["positional_scores"].cpu().numpy(), hh["positional_scores"].cpu().numpy(), atol=1e-4)


@pytest.mark.parametrize("name", ["gpt2", "txdec"])
def test_eager_capture_and_replay_give_the_same_hypotheses(name, dev):
    """Uses 1, 2 and 3 of a session (eager, capture, replay): identical hypotheses.  Another strategy, or the same
    with other numbers, on the same decoder gets a session of its own."""
    from vidsitu_amd.seq_gen import DiverseBeamSearch, DiverseSiblingsSearch, SeqGenCustom

    lm, tok, vocab, sample, prefix = _setup(name, dev, 2)
    kw = dict(beam_size=4, max_len_b=12, min_len=1)
    outs = []
    for use in range(3):
        gen = SeqGenCustom([lm], tok, search_strategy=DiverseBeamSearch(tok, 2, 0.5), **kw)
        outs.append(gen._generate(sample, prefix_tokens=prefix))
        ses = list(lm.decoder._vs_search_sessions.values())[-1]
        assert ses.strategy == ("groups", 2, 0.5) and ses.uses == use + 1
        assert (len(ses.graphs) > 0) == (use >= 1)
    for o in outs[1:]:
        _assert_same(o, outs[0], 0.0)
    sessions = [ses]  # kept alive, so that `is` tells sessions apart after the cache (two entries) dropped one
    for other, key in ((dict(search_strategy=DiverseBeamSearch(tok, 2, 1.0)), ("groups", 2, 1.0)),
                       (dict(search_strategy=DiverseBeamSearch(tok, 4)), ("groups", 4, 0.5)),
                       (dict(search_strategy=DiverseSiblingsSearch(tok, 0.5)), ("siblings", 0.5)),
                       (dict(diversity_rate=1.0), ("siblings", 1.0)), (dict(), None)):
        SeqGenCustom([lm], tok, **kw, **other)._generate(sample, prefix_tokens=prefix)
        ses = list(lm.decoder._vs_search_sessions.values())[-1]
        assert ses.strategy == key and ses.uses == 1 and not ses.graphs
        assert not any(ses is s for s in sessions)
        sessions.append(ses)


def test_options_through_the_plugin_surface(dev):
    """`--gen.diverse_beam_groups` through `get_cfg` -> `EvalB_Gen.forward_one_batch` (a new SeqGenCustom per batch):
    every step of the generation goes through `vs_beam_diverse_step` with the configured numbers."""
    from vidsitu_amd import ops
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    cfg = get_cfg({"task_type": "vb_arg", "mdl.mdl_name": "sfpret_txed_vbarg", "mdl.tx_dec_type": "gpt2",
                   "mdl.gpt2_mdl_name": "gpt2-synth-tiny", "tx_dec.decoder_layers": 1, "synth.gpt2_vocab": 211,
                   "gen.beam_size": 4, "gen.max_len_b": 20, "gen.min_len": 18, "gen.diverse_beam_groups": 2,
                   "gen.diverse_beam_strength": 1.5})
    comm = synth_data.make_comm(cfg)
    sel = get_mdl_loss_eval(cfg)
    torch.manual_seed(0)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev).eval()
    batch = synth_data.synth_srl_batch(comm, bs=2, n_ev=5, seq_len=10, device=dev)
    evl = sel["evl"](cfg, comm, dev)
    tok = comm.gpt2_hf_tok
    seen, plain = [], ops.beam_diverse_step

    def spy(*a, **kw):
        seen.append(a[-3:])
        return plain(*a, **kw)

    ops.beam_diverse_step = spy
    try:
        out = evl.forward_one_batch(mdl, batch)
    finally:
        ops.beam_diverse_step = plain
    seqs = [[t for t in ev["tokens"] if t != tok.pad_token_id] for r in out for ev in r["vb_output"].values()]
    assert len(seqs) == 10 and min(len(s) for s in seqs) >= 18
    assert len(seen) >= 18 and set(seen) == {(2, 1.5, 0.0)}


def test_main_dist_vb_arg_row_evaluates_with_diverse_groups(dev, tmp_path):
    """Beside the SRL row of test_gpu_main_dist.py: the same entry point with `--gen.beam_size=4
    --gen.diverse_beam_groups=2` runs its validation by diverse beam search."""
    from test_gpu_main_dist import _run

    rc, out, err = _run(["main_dist.py", "t_srl_s", "--task_type=vb_arg", "--mdl.mdl_name=sfpret_txe_txd_vbarg",
                         "--mdl.tx_dec_type=txdec", "--train.bs=2", "--ds.vsitu.num_ev=2", "--train.lr=1e-4",
                         "--overfit_batch=True", "--gen.beam_size=4", "--gen.max_len_b=8",
                         "--gen.diverse_beam_groups=2", f"--misc.tmp_path={tmp_path}", "--steps=2"], timeout=600)
    assert rc == 0, out[-3000:] + err
    assert "valid" in out, out
