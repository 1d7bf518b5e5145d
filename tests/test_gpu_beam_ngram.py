"""n-gram blocking (`gen.no_repeat_ngram_size`) on the GPU: the ban inside the scoring kernels
(`vs_beam_topk_ngram`, both the one-block and the sliced shape) against the reference's dict of n-grams
restated in numpy (tests/beam_ngram_ref.py), the two searches of `vidsitu_amd.seq_gen` against the oracle
search with the ban, per-step graphs included, and the option through the plugin surface.
Tolerances as in test_gpu_gpt2.py: token ids equal, finite scores within 2e-5 (kernel) / 1e-4 (search),
the -inf pattern equal."""
import glob
import os

import numpy as np
import pytest
import torch

import beam_ngram_ref as R
from oracle import beam_ref, gpt2_ref

pytestmark = pytest.mark.gpu
GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "gpt2_*.npz")))

ROWS, K = 6, 10
_rules_cache = {}


def _rules_inputs(V):
    """Logits, cumulative scores, forced tokens and the numpy scores after every rule but the ban, per
    `flags` (the inputs of test_gpu_gpt2.py::test_beam_topk_kernel_rules), computed once per V."""
    if V not in _rules_cache:
        rs = np.random.RandomState(0)
        pad, eos, unk = V - 1, V - 2, 5
        x = rs.randn(ROWS, V).astype(np.float32) * 3
        x[0, 17] = x[0, 400]
        x[4, V - 3] = x[4, 2] = 30.0
        x[1, 3] = np.nan
        cum = rs.randn(ROWS).astype(np.float32)
        cum[5] = -np.inf
        forced = np.array([-1, -1, 42, pad, -1, -1], dtype=np.int64)
        lps = {}
        for flags in (0, 1, 2):
            lp = beam_ref.log_softmax(x / np.float32(0.7))
            lp[lp != lp] = -np.inf
            lp[:, pad] = -np.inf
            lp[:, unk] -= 0.25
            if flags & 1:
                lp[:, :eos] = -np.inf
                lp[:, eos + 1:] = -np.inf
            for r in range(ROWS):
                if forced[r] >= 0 and forced[r] != pad:
                    keep = lp[r, forced[r]]
                    lp[r] = -np.inf
                    lp[r, forced[r]] = keep
                elif flags & 2:
                    lp[r, eos] = -np.inf
            lps[flags] = lp
        _rules_cache[V] = (x, cum, forced, lps, pad, eos, unk)
    return _rules_cache[V]


def _history(rs, V, n, step, L, targets):
    """One row of width L: positions 0..step end in the suffix (7, 8, 9)[:n-1], and each target token
    follows an earlier occurrence of that suffix; random filler in front (cut from the left when the
    step is too early to hold it all).  Positions after `step` are pad."""
    s = [7, 8, 9][: n - 1]
    body = []
    for t in targets:
        body += s + [t]
    body += s
    body = list(rs.randint(4, 200, size=max(0, step + 1 - len(body)))) + body
    row = np.full(L, V - 1, dtype=np.int64)
    row[: step + 1] = body[len(body) - (step + 1):]
    return row


@pytest.mark.parametrize("n", [1, 2, 3, 4])
# one block per row / 3 and 25 slices per row; 2048 | 2049: the last one-block V and the first sliced one,
# where the banned tokens 2047 and 2048 are the row's last (pad) and one past it | the two sides of the cut
@pytest.mark.parametrize("V", [1000, 5000, 50259, 2048, 2049])
def test_ngram_ban_kernel_rules(V, n, dev):
    from vidsitu_amd import ops

    x, cum, forced, lps, pad, eos, unk = _rules_inputs(V)
    b = 2047 if V >= 2048 else 31  # last token of a slice (of a bitmap word in the one-block kernel)
    top = int(beam_ref.topk_lowest_index(lps[0] + cum[:, None], 1)[1][1, 0])  # row 1's best without a ban
    targets = [[b, b + 1, 5, V - 3],        # both sides of a boundary, several bans, several slices
               [top, 400],                  # the row's arg-max
               [42],                        # the forced token: the row comes back all -inf
               [eos, 17],
               [2, V - 3, V + 5, -1],       # the tie across slices; ids outside [0, V) are ignored
               [3]]
    # (row width, step): step + 2 - n below 0 (nothing banned), step == n - 2 (the suffix has no earlier
    # occurrence yet), the first steps with one, a step in the middle, the last one the row has room
    # for, and a history of the longest search (more start positions than threads)
    cases = sorted({(40, s) for s in (n - 3, n - 2, n - 1, n, 25, 38) if s >= 0}) + [(1025, 1023)]
    xd, cumd, forcedd = (torch.from_numpy(a).to(dev) for a in (x, cum, forced))
    saw = {"none": False, "many": False, "boundary": False, "slices": False, "top": False, "forced": False}
    rs = np.random.RandomState(V + n)
    for L, step in cases:
        hist = np.stack([_history(rs, V, n, step, L, targets[r]) for r in range(ROWS)])
        bans = [[t for t in R.live(R.banned_ref(hist[r], step, n), pad) if 0 <= t < V] for r in range(ROWS)]
        if step + 2 - n < 0:
            assert not any(bans)
            saw["none"] = True
        # row 0's coverage is judged on what the kernel is handed, pad and ids >= V included: at V = 2048 | 2049
        # the banned 2047 and 2048 are pad / out of range, and the kernel must still index its bitmaps right
        raw0 = set(int(t) for t in R.banned_ref(hist[0], step, n))
        assert set(bans[0]) == {t for t in raw0 if 0 <= t < V and t != pad}
        saw["many"] |= len(raw0) >= 3
        saw["boundary"] |= b in raw0 and b + 1 in raw0
        saw["slices"] |= len({t // 2048 for t in raw0 if 0 <= t < V}) >= (2 if V > 2048 else 1)
        saw["top"] |= top in bans[1]
        saw["forced"] |= 42 in bans[2]
        # the device rows carry valid token ids after `step` (the search's buffers are uninitialised
        # there), in a buffer wider than the row: tok_ld is the pitch, not the width
        wide = rs.randint(0, V, size=(ROWS, L + 3)).astype(np.int64)
        wide[:, : step + 1] = hist[:, : step + 1]
        tok = torch.from_numpy(wide).to(dev)[:, :L]
        for flags in (0, 1, 2):
            lp = lps[flags].copy()
            for r in range(ROWS):
                lp[r, bans[r]] = -np.inf
            want_v, want_i = beam_ref.topk_lowest_index(lp + cum[:, None], K)
            v, i = ops.beam_topk(xd, cumd, forcedd, K, pad, eos, unk, unk_penalty=0.25, temperature=0.7,
                                 eos_only=bool(flags & 1), ban_eos=bool(flags & 2), tokens=tok, step=step,
                                 no_repeat_ngram_size=n)
            v, i = v.cpu().numpy(), i.cpu().numpy()
            what = f"V {V} n {n} L {L} step {step} flags {flags}"
            assert np.array_equal(i, want_i), what
            fin = np.isfinite(want_v)
            assert np.allclose(v[fin], want_v[fin], atol=2e-5), what
            assert np.array_equal(np.isneginf(v), np.isneginf(want_v)), what
            if 42 in bans[2]:
                assert np.isneginf(v[2]).all(), what
    assert saw["none"] == (n >= 3) and all(saw[key] for key in saw if key != "none"), saw


@pytest.mark.parametrize("V", [1000, 5000, 50259])
def test_no_ban_gives_the_bits_of_vs_beam_topk(V, dev):
    from vidsitu_amd import _lib, ops

    x, cum, forced, lps, pad, eos, unk = _rules_inputs(V)
    xd, cumd, forcedd = (torch.from_numpy(a).to(dev) for a in (x, cum, forced))
    tok = torch.from_numpy(np.random.RandomState(1).randint(0, V, size=(ROWS, 40)).astype(np.int64)).to(dev)
    tok[:, 20:30] = tok[:, 5:15]  # positions 28, 29 repeat 13, 14: with n = 3 position 15 is banned at step 29 ...
    tok[:, 15] = ops.beam_topk(xd, cumd, forcedd, K, pad, eos, unk, unk_penalty=0.25, temperature=0.7)[1][:, 0]
    # ... and holds every row's best token
    for flags in (0, 1, 2):
        kw = dict(unk_penalty=0.25, temperature=0.7, eos_only=bool(flags & 1), ban_eos=bool(flags & 2))
        v0, i0 = ops.beam_topk(xd, cumd, forcedd, K, pad, eos, unk, **kw)
        v1 = torch.empty_like(v0)
        i1 = torch.empty_like(i0)
        ws = torch.empty(int(_lib.load().vs_beam_topk_workspace_bytes(ROWS, V, K)), dtype=torch.uint8, device=dev)
        _lib.call("vs_beam_topk_ngram", ops._ptr(xd), ops._ptr(cumd), ops._ptr(forcedd), ops._ptr(tok), 40, 29, 0,
                  ops._ptr(v1), ops._ptr(i1), ROWS, V, K, pad, eos, unk, 0.25, 0.7, flags, ops._ptr(ws),
                  ws.numel(), ops._stream())
        assert torch.equal(i1, i0) and torch.equal(v1.view(torch.int32), v0.view(torch.int32))
        a = ops.beam_topk(xd, cumd, forcedd, K, pad, eos, unk, tokens=tok, step=29, no_repeat_ngram_size=3, **kw)
        c = ops.beam_topk(xd, cumd, forcedd, K, pad, eos, unk, tokens=tok, step=29, no_repeat_ngram_size=3, **kw)
        assert torch.equal(a[1], c[1]) and torch.equal(a[0].view(torch.int32), c[0].view(torch.int32))
        if flags == 0:
            assert not torch.equal(a[1], i0)  # and the ban did change the lists


def test_wrapper_checks_the_token_history(dev):
    from vidsitu_amd import _lib, ops

    x = torch.randn(2, 50, device=dev)
    for bad in (None, torch.zeros(2, 8, dtype=torch.int32, device=dev), torch.zeros(3, 8, dtype=torch.long, device=dev),
                torch.zeros(2, 16, dtype=torch.long, device=dev)[:, ::2]):
        with pytest.raises(_lib.VsError):
            ops.beam_topk(x, None, None, 4, 1, 2, 3, tokens=bad, step=0, no_repeat_ngram_size=2)
    with pytest.raises(_lib.VsError):
        ops.beam_topk(x, None, None, 4, 1, 2, 3, tokens=torch.zeros(2, 8, dtype=torch.long, device=dev), step=8,
                      no_repeat_ngram_size=2)


class _Tok:
    def __init__(self, vocab, pad, eos, unk):
        self.v, self._pad, self._eos, self._unk = vocab, pad, eos, unk
        self.pad_token_id, self.eos_token_id = pad, eos

    def __len__(self):
        return self.v

    def pad(self):
        return self._pad

    def eos(self):
        return self._eos

    def unk(self):
        return self._unk


class _StubDecoder(torch.nn.Module):
    """Logits from two tables (tests/beam_ngram_ref.py::stub_step_logits): both sides of the comparison
    see the same fp32 logits, so only the rounding of the log-softmax separates them."""

    def __init__(self, table, hist, dev):
        super().__init__()
        self.table, self.hist = torch.from_numpy(table).to(dev), torch.from_numpy(hist).to(dev)

    def forward(self, tokens, encoder_out=None, incremental_state=None):
        h = (tokens * torch.arange(1, tokens.shape[1] + 1, device=tokens.device)).sum(1) % 101
        return ((self.table[tokens[:, -1]] + self.hist[h]).unsqueeze(1),)


class _StubLM(torch.nn.Module):
    def __init__(self, decoder):
        super().__init__()
        self.use_encoder = False
        self.decoder = decoder

    def max_decoder_positions(self):
        return 1024

    def forward_encoder(self, inp):
        return None


def _toks(fin):
    return [[h["tokens"].tolist() for h in sent] for sent in fin]


def _assert_search_equals(got, want):
    assert _toks(got) == _toks(want)
    for sg, sw in zip(got, want):
        for hg, hw in zip(sg, sw):
            assert abs(float(hg["score"]) - hw["score"]) < 1e-4
            assert np.allclose(hg["positional_scores"].cpu().numpy(), hw["positional_scores"], atol=1e-4)


_stub_cache = {}


def _stub_oracle(V, seed, n):
    """The oracle's search of one stub case, once for both arms."""
    if (V, seed, n) not in _stub_cache:
        table, hist, prefix = R.stub_tables(V, seed, 2)
        kw = dict(bsz=2, vocab=V, pad=1, eos=2, unk=3, beam_size=3, max_len_b=16, min_len=6,
                  prefix_tokens=prefix)
        step_logits = R.stub_step_logits(table, hist)
        plain = beam_ref.generate(step_logits, **kw)
        _stub_cache[V, seed, n] = (table, hist, prefix, plain) + R.generate(step_logits, n, **kw)
    return _stub_cache[V, seed, n]


@pytest.mark.parametrize("device_search", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("V,seed", [(12, 2), (40, 4)])
def test_search_with_a_ban_equals_the_oracle_on_a_stub_decoder(V, seed, n, device_search, dev):
    from vidsitu_amd.seq_gen import SeqGenCustom

    table, hist, prefix, plain, want, bans, gap = _stub_oracle(V, seed, n)
    # what keeps the comparison honest: no choice within rounding of another, the ban acts and matters
    print(f"V {V} seed {seed} n {n}: {bans} live bans, smallest gap {gap:.3e}")
    assert gap >= 1e-3 and bans >= 1
    assert any(a != b for a, b in zip(_toks(want), _toks(plain)))
    gen = SeqGenCustom([_StubLM(_StubDecoder(table, hist, dev))], _Tok(V, 1, 2, 3), beam_size=3, max_len_b=16,
                       min_len=6, no_repeat_ngram_size=n, use_kv_cache=False, device_search=device_search)
    sample = {"src_tokens": torch.zeros(2, 1, dtype=torch.long, device=dev),
              "src_lengths": torch.ones(2, dtype=torch.long, device=dev)}
    got = gen._generate(sample, prefix_tokens=torch.from_numpy(prefix).to(dev))
    _assert_search_equals(got, want)


def test_device_search_graphs_with_a_ban_equal_the_oracle(dev):
    """Four uses of one session on the GPT-2 slice with a KV cache (eager, capture, replay, replay), n = 2,
    two prefix sets in turn; then n = 0 on the same decoder gets a session of its own."""
    from test_gpu_gpt2 import _LM, _model_from_golden
    from vidsitu_amd.seq_gen import SeqGenCustom

    z, w, n_head, m = _model_from_golden(GOLD[0], dev)
    vocab = int(z["dims"][0])
    pad, eos, unk = vocab - 1, vocab - 2, vocab - 2
    w = dict(w)
    w["transformer.wte.weight"] = w["transformer.wte.weight"].copy()
    w["transformer.wte.weight"][eos] *= 3.0
    with torch.no_grad():
        m.P("transformer.wte.weight")[eos] *= 3.0
    bsz, beam = 4, 3
    lm = _LM(m, pad)

    def step_logits(tokens, sent_ids):
        return gpt2_ref.forward(w, tokens, (tokens != pad).astype(np.int64), n_head)[:, -1, :]

    sample = {"src_tokens": torch.zeros(bsz, 1, dtype=torch.long, device=dev),
              "src_lengths": torch.ones(bsz, dtype=torch.long, device=dev)}
    tok = _Tok(vocab, pad, eos, unk)
    refs = []
    for first in (5, 6):
        prefix = np.array([[first], [9], [5], [70]], dtype=np.int64)
        kw = dict(bsz=bsz, vocab=vocab, pad=pad, eos=eos, unk=unk, beam_size=beam, max_len_b=12, min_len=1,
                  prefix_tokens=prefix, max_decoder_positions=int(z["dims"][1]) - 1)
        plain = beam_ref.generate(step_logits, **kw)
        want, bans, gap = R.generate(step_logits, 2, **kw)
        print(f"prefix {prefix.ravel().tolist()}: {bans} live bans, smallest gap {gap:.3e}")
        assert gap >= 1e-3 and bans >= 1 and any(a != b for a, b in zip(_toks(want), _toks(plain)))
        refs.append((prefix, plain, want))
    for use in range(4):
        prefix, _, want = refs[use % 2]
        gen = SeqGenCustom([lm], tok, beam_size=beam, max_len_b=12, min_len=1, no_repeat_ngram_size=2)
        got = gen._generate(sample, prefix_tokens=torch.from_numpy(prefix).to(dev))
        ses = list(lm.decoder._vs_search_sessions.values())[-1]
        assert ses.ngram == 2 and ses.uses == use + 1 and (len(ses.graphs) > 0) == (use >= 1)
        _assert_search_equals(got, want)
    prefix, plain, _ = refs[0]
    gen = SeqGenCustom([lm], tok, beam_size=beam, max_len_b=12, min_len=1)
    got = gen._generate(sample, prefix_tokens=torch.from_numpy(prefix).to(dev))
    sessions = list(lm.decoder._vs_search_sessions.values())
    assert len(sessions) == 2 and sessions[-1].ngram == 0 and sessions[-1].uses == 1 and sessions[0] is ses
    _assert_search_equals(got, plain)


def _bigram_repeats(out, pad, bos):
    reps = []
    for rec in out:
        for ev in rec["vb_output"].values():
            toks = [t for t in ev["tokens"] if t != pad]
            reps.append(R.has_repeated_ngram([bos] + toks, 2))
    return reps


@pytest.mark.parametrize("dec", ["gpt2", "txdec"])
def test_option_through_the_plugin_surface(dec, dev):
    """`--gen.no_repeat_ngram_size 2` through `get_cfg` -> `EvalB_Gen.forward_one_batch`: no generated
    sequence repeats a bigram, where the same batch without the option does."""
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    outs = {}
    for n in (0, 2):
        over = {"task_type": "vb_arg", "mdl.mdl_name": "sfpret_txed_vbarg", "mdl.tx_dec_type": dec,
                "tx_dec.decoder_layers": 1, "synth.gpt2_vocab": 211, "gen.beam_size": 2, "gen.max_len_b": 26,
                "gen.min_len": 24, "gen.no_repeat_ngram_size": n}
        if dec == "gpt2":
            over["mdl.gpt2_mdl_name"] = "gpt2-synth-tiny"
        cfg = get_cfg(over)
        assert cfg.gen.no_repeat_ngram_size == n
        comm = synth_data.make_comm(cfg)
        sel = get_mdl_loss_eval(cfg)
        torch.manual_seed(0)
        mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev).eval()
        batch = synth_data.synth_srl_batch(comm, bs=2, n_ev=5, seq_len=10, device=dev)
        out = sel["evl"](cfg, comm, dev).forward_one_batch(mdl, batch)
        assert len(out) == 2 and all(len(r["vb_output"]) == 5 for r in out)
        tok = comm.gpt2_hf_tok
        outs[n] = _bigram_repeats(out, tok.pad_token_id, tok.eos_token_id)
        lens = [len([t for t in ev["tokens"] if t != tok.pad_token_id]) for r in out for ev in r["vb_output"].values()]
        print(f"{dec} n {n}: lengths {lens}, sequences with a repeated bigram {sum(outs[n])} of {len(outs[n])}")
        assert min(lens) >= 24  # long enough for the constraint to bind
    assert any(outs[0]), "the batch does not exercise the option: no repeated bigram without it"
    assert not any(outs[2])
