"""The sampling search of `vidsitu_amd.seq_gen` (`Sampling`, `gen.sampling*`) on the GPU: the step's bookkeeping
(`vs_sample_step`) against the numpy step of tests/sample_ref.py bit for bit; whole searches of the GPT-2 slice and the
tiny fairseq-style decoder against `sample_ref.search` fed with the device's own per-step logits (so the draws and the
bookkeeping are held to the restatement, not to themselves); host loop == device loop; eager / captured / replayed
steps after `reseed`; the stream continuing from one generation to the next; top-k 1 with one beam == beam search;
the n-gram ban; the options through the plugin surface and `main_dist.py`."""
import glob
import os

import numpy as np
import pytest
import torch

import beam_ngram_ref
import beam_step_ref
import sample_ref as SR

pytestmark = pytest.mark.gpu
GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "gpt2_*.npz")))
SEED = 77


def test_sample_step_equals_the_numpy_step(dev):
    """Synthetic draws (eos now and then, a -inf candidate, ignored beams drawing eos again) through every step of a
    search: tokens, scores, flags, finalized hypotheses, the reorder index and the ancestry table, bit for bit."""
    from vidsitu_amd import ops

    bsz, beam, max_len, V, pad, eos = 5, 3, 9, 50, 49, 48
    rs = np.random.RandomState(5)
    st = beam_step_ref.new_state(bsz, beam, max_len, pad, eos, anc_ld=max_len + 2)
    d = {k: (None if a is None else torch.from_numpy(a.copy()).to(dev)) for k, a in st.items()}
    saw_ignore = saw_neginf = False
    for step in range(max_len + 1):
        tok = rs.randint(0, V - 2, bsz * beam).astype(np.int64)
        tok[rs.rand(bsz * beam) < 0.25] = eos
        val = (st["sc"][:, step - 1] if step else 0) + np.log(rs.rand(bsz * beam)).astype(np.float32)
        val = val.astype(np.float32)
        if step == 2:
            val[4], tok[4] = -np.inf, 0
            saw_neginf = True
        if step == max_len:
            tok[:] = eos
        new, reorder = SR.step(st, val, tok, step, eos, max_len)
        out = {k: (None if a is None else torch.empty_like(a)) for k, a in d.items() if k in ("tok", "sc", "anc")}
        re_d = torch.empty(bsz * beam, dtype=torch.long, device=dev)
        ops.sample_step(torch.from_numpy(val).to(dev), torch.from_numpy(tok).to(dev), d["tok"], out["tok"], d["sc"],
                        out["sc"], d["ignore"], d["finished"], d["nfin"], d["remaining"], d["fin_tok"],
                        d["fin_score"], d["fin_pos"], d["fin_len"], re_d, bsz, beam, step, max_len, eos, True, 1.0,
                        anc_in=d["anc"], anc_out=out["anc"])
        d.update(out)
        saw_ignore |= bool(new["ignore"].any())
        live = np.repeat(1 - new["finished"], beam).astype(bool)  # rows of a finished sentence idle
        assert np.array_equal(re_d.cpu().numpy(), reorder), step
        for k in ("ignore", "finished", "nfin", "remaining", "fin_tok", "fin_len"):
            assert np.array_equal(d[k].cpu().numpy(), new[k]), (step, k)
        for k in ("fin_score", "fin_pos"):
            assert np.array_equal(d[k].cpu().numpy().view(np.uint32), new[k].view(np.uint32)), (step, k)
        assert np.array_equal(d["tok"].cpu().numpy()[live, : step + 2], new["tok"][live, : step + 2]), step
        assert np.array_equal(d["sc"].cpu().numpy()[live, : step + 1].view(np.uint32),
                              new["sc"][live, : step + 1].view(np.uint32)), step
        assert np.array_equal(d["anc"].cpu().numpy()[live, : step + 2], new["anc"][live, : step + 2]), step
        st = new
        if st["remaining"][0] == 0:
            break
    assert st["remaining"][0] == 0 and saw_ignore and saw_neginf and int(st["nfin"].min()) >= 1


# ---- the two decoders ---------------------------------------------------------------------------------------------
def _gpt2(dev):
    from test_gpu_gpt2 import _LM, _model_from_golden
    from test_gpu_beam_ngram import _Tok

    z, w, n_head, m = _model_from_golden(GOLD[0], dev)
    vocab = int(z["dims"][0])
    pad, eos = vocab - 1, vocab - 2
    with torch.no_grad():
        m.P("transformer.wte.weight")[eos] *= 3.0  # hypotheses finish at different steps
    return _LM(m, pad), _Tok(vocab, pad, eos, eos), vocab


def _txdec(dev, bsz):
    from test_gpu_txdec import D, VOC, _EncDec, _model, _Tok

    w, m = _model(dev, seed=9)
    with torch.no_grad():
        m.P("output_projection.weight")[VOC - 2] *= 2.5
    m.eval()
    enc = torch.randn(bsz, D, generator=torch.Generator().manual_seed(8))
    return _EncDec(m, enc.to(dev)), _Tok(), VOC


def _setup(name, dev, bsz):
    lm, tok, vocab = _gpt2(dev) if name == "gpt2" else _txdec(dev, bsz)
    sample = {"src_tokens": torch.zeros(bsz, 1, dtype=torch.long, device=dev),
              "src_lengths": torch.ones(bsz, dtype=torch.long, device=dev)}
    prefix = torch.tensor([[5], [9], [70]][:bsz], dtype=torch.long, device=dev)
    return lm, tok, vocab, sample, prefix


def _toks(fin):
    return [[[int(t) for t in h["tokens"]] for h in sent] for sent in fin]


def _scores(fin):
    return [[float(h["score"]) for h in sent] for sent in fin]


def _assert_same(got, want, tol):
    assert _toks(got) == _toks(want)
    for a, b in zip(sum(_scores(got), []), sum(_scores(want), [])):
        assert abs(a - b) <= tol, (a, b)


def _recorded(gen):
    """Make `gen` keep every decoder call's (prefix tokens, last-position logits) on the host."""
    calls = []
    plain = gen.model.decoder_logits

    def rec(tokens, encoder_outs, state):
        out = plain(tokens, encoder_outs, state)
        calls.append((tokens.cpu().numpy().copy(), out.float().cpu().numpy().copy()))
        return out

    gen.model.decoder_logits = rec
    return calls


def _reference(calls, tok, vocab, bsz, step0, prefix, **kw):
    """`sample_ref.search` on the device's own logits: the step callback refuses rows the device did not have."""
    def step_logits(tokens, sent_ids):
        t, logits = calls[tokens.shape[1] - 1]
        assert np.array_equal(t, tokens), f"the searches part before step {tokens.shape[1] - 1}"
        return logits

    return SR.search(step_logits, bsz, vocab, tok.pad(), tok.eos(), tok.unk(), SEED, step0=step0,
                     prefix_tokens=prefix.cpu().numpy(), **kw)


def _stream_step(lm):
    (stream,) = lm.decoder._vs_sample_streams.values()
    return int(stream.state.cpu()[1])


@pytest.mark.parametrize("knobs", [dict(), dict(sampling_topk=5), dict(sampling_topp=0.9),
                                   dict(sampling_topp=0.9, no_repeat_ngram_size=3)],
                         ids=["plain", "topk5", "topp0.9", "topp0.9-ngram3"])
@pytest.mark.parametrize("name", ["gpt2", "txdec"])
def test_device_search_equals_the_restatement(name, knobs, dev):
    """Two generations in a row without a KV cache (every step eager, so the logits can be recorded): the first draws
    from steps 0.. of the seed, the second goes on where the first one's ticks ended."""
    from vidsitu_amd.seq_gen import SeqGenCustom

    bsz, beam = 3, 3
    lm, tok, vocab, sample, prefix = _setup(name, dev, bsz)
    kw = dict(beam_size=beam, max_len_b=12, min_len=2, **knobs)
    firsts = []
    for use in range(2):
        gen = SeqGenCustom([lm], tok, sampling=True, seed=SEED, use_kv_cache=False, **kw)
        if use == 0:
            gen.reseed(SEED)
        step0 = _stream_step(lm) if use else 0
        calls = _recorded(gen)
        got = gen._generate(sample, prefix_tokens=prefix)
        assert _stream_step(lm) == step0 + len(calls)  # one tick per search step
        want, nsteps = _reference(calls, tok, vocab, bsz, step0, prefix, **kw)
        assert nsteps <= len(calls)
        _assert_same(got, want, 1e-5)
        assert all(len(s) == beam for s in got)
        if knobs.get("no_repeat_ngram_size"):
            assert not any(beam_ngram_ref.has_repeated_ngram([tok.eos()] + h, 3) for s in _toks(got) for h in s)
        firsts.append(_toks(got))
    assert firsts[0] != firsts[1]  # the second generation drew from other words


@pytest.mark.parametrize("name,kv", [("gpt2", True), ("gpt2", False), ("txdec", True)])
def test_host_search_equals_device_search(name, kv, dev):
    from vidsitu_amd.seq_gen import SeqGenCustom

    lm, tok, vocab, sample, prefix = _setup(name, dev, 3)
    outs = []
    for device_search in (True, False):
        gen = SeqGenCustom([lm], tok, beam_size=3, max_len_b=12, min_len=1, sampling=True, sampling_topp=0.9, seed=SEED,
                           use_kv_cache=kv, device_search=device_search)
        gen.reseed(SEED)
        outs.append(gen._generate(sample, prefix_tokens=prefix))
    # the host loop drops finished sentences from the batch, so its decoder runs at other row counts than the device
    # search's and rounds its logits otherwise: the search tolerance of test_gpu_gpt2.py (1e-4), tokens equal
    _assert_same(outs[1], outs[0], 1e-4)
    for hd, hh in zip(sum(outs[0], []), sum(outs[1], [])):
        assert np.allclose(hd["positional_scores"].cpu().numpy(), hh["positional_scores"].cpu().numpy(), atol=1e-4)


@pytest.mark.parametrize("name", ["gpt2", "txdec"])
def test_eager_capture_and_replay_draw_the_same_after_reseed(name, dev):
    """Uses 1, 2 and 3 of a session (eager, capture, replay), each from step 0 of the seed: identical hypotheses.  A
    fourth use without `reseed` goes on in the stream and draws other tokens; a `SeqGenCustom` built anew (as
    EvalB_Gen does per batch) continues the decoder's stream instead of restarting it."""
    from vidsitu_amd.seq_gen import Sampling, SeqGenCustom

    lm, tok, vocab, sample, prefix = _setup(name, dev, 2)
    outs = []
    for use in range(4):
        gen = SeqGenCustom([lm], tok, beam_size=3, max_len_b=12, min_len=1, seed=SEED,
                           search_strategy=Sampling(tok, sampling_topk=40))
        if use < 3:
            gen.reseed(SEED)
        else:
            assert _stream_step(lm) > 0
        outs.append(gen._generate(sample, prefix_tokens=prefix))
        ses = list(lm.decoder._vs_search_sessions.values())[-1]
        assert ses.strategy == (40, -1.0) and ses.uses == use + 1
        # both decoders keep a KV cache and read no encoder output in a step (`uses_encoder_out = False`): both capture
        assert (len(ses.graphs) > 0) == (use >= 1)
    for o in outs[1:3]:
        _assert_same(o, outs[0], 0.0)
    assert _toks(outs[3]) != _toks(outs[0])


@pytest.mark.parametrize("name", ["gpt2", "txdec"])
def test_a_generator_that_names_another_seed_restarts_the_stream_on_every_use(name, dev):
    """`for s in seeds: SeqGenCustom(..., seed=s).generate(...)` on one decoder: use 1 of the session is eager, use 2
    captures its steps, uses 3 and 4 replay them -- and each draws from step 0 of its own seed, as a generator does
    that is told `reseed(s)` on a second copy of the decoder."""
    from vidsitu_amd.seq_gen import SeqGenCustom

    lm, tok, vocab, sample, prefix = _setup(name, dev, 2)
    lm2 = _setup(name, dev, 2)[0]
    kw = dict(beam_size=3, max_len_b=12, min_len=1, sampling=True, sampling_topp=0.9)
    outs = []
    for use, seed in enumerate([SEED, SEED + 1, SEED + 2, SEED + 1]):
        got = SeqGenCustom([lm], tok, seed=seed, **kw)._generate(sample, prefix_tokens=prefix)
        ses = list(lm.decoder._vs_search_sessions.values())[-1]
        assert ses.uses == use + 1 and (len(ses.graphs) > 0) == (use >= 1)
        ref = SeqGenCustom([lm2], tok, seed=SEED, **kw)
        ref.reseed(seed)
        _assert_same(got, ref._generate(sample, prefix_tokens=prefix), 0.0)
        outs.append(_toks(got))
    assert outs[1] == outs[3] and outs[0] != outs[1] and outs[1] != outs[2]


def test_topk_1_with_one_beam_is_the_beam_search(dev):
    from vidsitu_amd.seq_gen import SeqGenCustom

    lm, tok, vocab, sample, prefix = _setup("gpt2", dev, 3)
    kw = dict(beam_size=1, max_len_b=12, min_len=1)
    want = SeqGenCustom([lm], tok, **kw)._generate(sample, prefix_tokens=prefix)
    got = SeqGenCustom([lm], tok, sampling=True, sampling_topk=1, seed=SEED, **kw)._generate(sample, prefix_tokens=prefix)
    _assert_same(got, want, 1e-6)


def test_options_through_the_plugin_surface(dev):
    """`--gen.sampling` / `--gen.sampling_topk` / `--gen.seed` / `--gen.no_repeat_ngram_size` through `get_cfg` ->
    `EvalB_Gen.forward_one_batch` (a new SeqGenCustom per batch): no generated sequence repeats a 3-gram, and two
    batches in a row draw different captions for the same events."""
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    cfg = get_cfg({"task_type": "vb_arg", "mdl.mdl_name": "sfpret_txed_vbarg", "mdl.tx_dec_type": "gpt2",
                   "mdl.gpt2_mdl_name": "gpt2-synth-tiny", "tx_dec.decoder_layers": 1, "synth.gpt2_vocab": 211,
                   "gen.beam_size": 2, "gen.max_len_b": 20, "gen.min_len": 18, "gen.sampling": True,
                   "gen.sampling_topk": 40, "gen.seed": 5, "gen.no_repeat_ngram_size": 3})
    comm = synth_data.make_comm(cfg)
    sel = get_mdl_loss_eval(cfg)
    torch.manual_seed(0)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev).eval()
    batch = synth_data.synth_srl_batch(comm, bs=2, n_ev=5, seq_len=10, device=dev)
    evl = sel["evl"](cfg, comm, dev)
    tok = comm.gpt2_hf_tok
    seqs = []
    for _ in range(2):
        out = evl.forward_one_batch(mdl, batch)
        seqs.append([[t for t in ev["tokens"] if t != tok.pad_token_id] for r in out for ev in r["vb_output"].values()])
        assert len(seqs[-1]) == 10 and min(len(s) for s in seqs[-1]) >= 18
        assert not any(beam_ngram_ref.has_repeated_ngram([tok.eos_token_id] + s, 3) for s in seqs[-1])
    assert seqs[0] != seqs[1]


def test_main_dist_vb_arg_row_evaluates_with_nucleus_sampling(dev, tmp_path):
    """Beside the SRL row of test_gpu_main_dist.py: the same entry point with `--gen.sampling=True
    --gen.sampling_topp=0.9` runs its validation by sampling search."""
    from test_gpu_main_dist import _run

    rc, out, err = _run(["main_dist.py", "t_srl_s", "--task_type=vb_arg", "--mdl.mdl_name=sfpret_txe_txd_vbarg",
                         "--mdl.tx_dec_type=txdec", "--train.bs=2", "--ds.vsitu.num_ev=2", "--train.lr=1e-4",
                         "--overfit_batch=True", "--gen.beam_size=2", "--gen.max_len_b=8", "--gen.sampling=True",
                         "--gen.sampling_topp=0.9", f"--misc.tmp_path={tmp_path}", "--steps=2"], timeout=600)
    assert rc == 0, out[-3000:] + err
    assert "valid" in out, out
