"""`vs_beam_step` against the step-level restatement of the reference (tests/beam_step_ref.py), bit for
bit, and the two searches of `vidsitu_amd.seq_gen` against the oracle on a table-lookup decoder.

Step level: the candidate lists are scripted on an exact grid (tests/beam_cases.py: multiples of 2^-6,
every cumulative sum exact in fp32), so kernel and restatement see identical numbers, designed ties are
real ties and nothing needs a tolerance -- except `fin_score` under a length penalty other than 0 or 1,
where `powf` (documented to 1 ulp) meets a correctly rounded double power and each side rounds its
quotient once: 4 ulp of the fp32 result.  The kernel is chained on its own outputs, the restatement on
its own, and every buffer is compared after every step.  tests/test_beam_step_ref.py anchors the
restatement on the oracle and asserts which case reaches which branch.

Whole searches: tokens equal, scores and positional scores within 1e-4 (the tolerance of the search
tests in test_gpu_gpt2.py); the CPU test asserts that every case is decidable at that precision."""
import numpy as np
import pytest
import torch

import beam_cases as C
import beam_step_ref as S

pytestmark = pytest.mark.gpu


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(_bits(got), _bits(want)), what


@pytest.mark.parametrize("name", list(C.STEP_CASES))
def test_vs_beam_step_equals_the_restatement(name, dev):
    from vidsitu_amd import ops

    c = C.STEP_CASES[name]
    bsz, beam, V, max_len = c["bsz"], c["beam"], c["V"], c["max_len"]
    rows, Lt = bsz * beam, max_len + 2
    eos = V - 2
    k = min(2 * beam, V - 1)
    steps, start = [], {}
    C.run_step_case(c, on_step=lambda *a: steps.append(a), on_start=lambda st: start.update(st))

    d = {key: (None if a is None else torch.from_numpy(a).to(dev)) for key, a in start.items()}
    tok = [d["tok"], torch.empty_like(d["tok"])]
    sc = [d["sc"], torch.empty_like(d["sc"])]
    anc = None if d["anc"] is None else [d["anc"], torch.empty_like(d["anc"])]
    reorder = torch.empty(rows, dtype=torch.long, device=dev)
    exact_score = (not c["normalize"]) or c["len_penalty"] in (0.0, 1.0)
    for step, row_val, row_idx, want, want_reorder in steps:
        assert row_val.shape == (rows, k) and row_val.dtype == np.float32
        cur = step & 1
        tok[1 - cur].fill_(-5)
        sc[1 - cur].fill_(77.0)
        reorder.fill_(-1)
        if anc is not None:
            anc[1 - cur].fill_(-9)
        ops.beam_step(torch.from_numpy(row_val).to(dev), torch.from_numpy(row_idx).to(dev), tok[cur], tok[1 - cur],
                      sc[cur], sc[1 - cur], d["ignore"], d["finished"], d["nfin"], d["remaining"], d["fin_tok"],
                      d["fin_score"], d["fin_pos"], d["fin_len"], reorder, bsz, beam, k, V, step, max_len, eos,
                      c["normalize"], c["len_penalty"], anc_in=None if anc is None else anc[cur],
                      anc_out=None if anc is None else anc[1 - cur])
        what = f"{name} step {step}"
        _same(tok[1 - cur], want["tok"], what + " tok")
        _same(sc[1 - cur], want["sc"], what + " sc")
        for key in ("ignore", "finished", "nfin", "remaining", "fin_tok", "fin_pos", "fin_len"):
            _same(d[key], want[key], f"{what} {key}")
        _same(reorder, want_reorder, what + " reorder")
        if anc is not None:
            got = anc[1 - cur].cpu().numpy()
            assert np.array_equal(got[:, : step + 2], want["anc"][:, : step + 2]), what + " anc"
            assert (got[:, step + 2:] == -9).all(), what + " anc: written past position step + 1"
        if exact_score:
            _same(d["fin_score"], want["fin_score"], what + " fin_score")
        else:
            got, ref = d["fin_score"].cpu().numpy(), want["fin_score"]
            done = want["fin_len"] != C.SENTINEL["fin_len"]
            assert np.array_equal(_bits(got[~done]), _bits(ref[~done])), what + " fin_score: unfinalised slot"
            ulps = np.abs(got[done].astype(np.float64) - ref[done]) / np.spacing(np.abs(ref[done]))
            assert np.all(ulps <= 4), f"{what} fin_score: {ulps.max()} ulp"
    assert int(d["remaining"]) == 0


def test_vs_beam_step_refuses_what_it_cannot_hold(dev):
    from vidsitu_amd import _lib, ops

    st = S.new_state(1, 33, 4, 99, 98)
    d = {key: torch.from_numpy(a).to(dev) for key, a in st.items() if a is not None}
    out = torch.empty(33, dtype=torch.long, device=dev)
    rv, ri = torch.zeros(33, 64, device=dev), torch.zeros(33, 64, dtype=torch.long, device=dev)
    for beam, k in ((33, 64), (32, 65), (32, 0)):
        with pytest.raises(_lib.VsError):
            ops.beam_step(rv, ri, d["tok"], d["tok"].clone(), d["sc"], d["sc"].clone(), d["ignore"], d["finished"],
                          d["nfin"], d["remaining"], d["fin_tok"], d["fin_score"], d["fin_pos"], d["fin_len"], out,
                          1, beam, k, 100, 0, 4, 98, True, 1.0)


# ---- whole searches on a table-lookup decoder -----------------------------------------------------------
class _Tok:
    def __init__(self, vocab, pad, eos, unk):
        self.v, self._pad, self._eos, self._unk = vocab, pad, eos, unk

    def __len__(self):
        return self.v

    def pad(self):
        return self._pad

    def eos(self):
        return self._eos

    def unk(self):
        return self._unk


class _HashDecoder(torch.nn.Module):
    """tests/beam_cases.py::hash_step_logits in torch integer ops on the device (capturable in a graph):
    the last position's logits are two table rows chosen by a hash of the row's whole history.  The
    incremental state is accepted and ignored."""
    uses_encoder_out = False

    def __init__(self, a, b, w, dev):
        super().__init__()
        self.a, self.b, self.w = (torch.from_numpy(t).to(dev) for t in (a, b, w))

    def forward(self, tokens, encoder_out=None, incremental_state=None):
        h = ((tokens + 1) * self.w[: tokens.shape[1]]).sum(1) % (C.HASH_A * C.HASH_B)
        return ((self.a[h % C.HASH_A] + self.b[torch.div(h, C.HASH_A, rounding_mode="floor")]).unsqueeze(1),)

    def reorder_incremental_state(self, state, new_order):
        pass


class _LM(torch.nn.Module):
    def __init__(self, decoder):
        super().__init__()
        self.use_encoder = False
        self.decoder = decoder

    def max_decoder_positions(self):
        return 1024

    def forward_encoder(self, inp):
        return None


def _assert_search_equals(got, want, what):
    assert [[h["tokens"].tolist() for h in s] for s in got] == [[h["tokens"].tolist() for h in s] for s in want], what
    for sg, sw in zip(got, want):
        for hg, hw in zip(sg, sw):
            assert abs(float(hg["score"]) - hw["score"]) < 1e-4, what
            assert np.allclose(hg["positional_scores"].cpu().numpy(), hw["positional_scores"], atol=1e-4), what


@pytest.mark.parametrize("name", list(C.SEARCH_CASES))
def test_searches_equal_the_oracle_on_a_scripted_decoder(name, dev):
    """Device search with a KV-cache state three times (eager, one hipGraph per step captured, replayed)
    and once without, then the host loop: all five return the oracle's hypotheses."""
    from vidsitu_amd.seq_gen import SeqGenCustom

    c = C.SEARCH_CASES[name]
    a, b, w, prefix, kw = C.search_inputs(c)
    want = C.search_oracle(name)
    lm = _LM(_HashDecoder(a, b, w, dev))
    sample = {"src_tokens": torch.zeros(c["bsz"], 1, dtype=torch.long, device=dev),
              "src_lengths": torch.ones(c["bsz"], dtype=torch.long, device=dev)}
    pre = None if prefix is None else torch.from_numpy(prefix).to(dev)
    opts = dict(beam_size=c["beam"], max_len_b=c["max_len_b"], min_len=c["min_len"], unk_penalty=0.3, **c["kw"])
    for use in range(3):
        gen = SeqGenCustom([lm], _Tok(c["V"], 1, 2, 3), use_kv_cache=True, device_search=True, **opts)
        got = gen._generate(sample, prefix_tokens=pre)
        ses = list(lm.decoder._vs_search_sessions.values())[-1]
        assert ses.uses == use + 1 and (len(ses.graphs) > 0) == (use >= 1)
        _assert_search_equals(got, want, f"{name} device, use {use + 1}")
    for device_search in (True, False):
        gen = SeqGenCustom([lm], _Tok(c["V"], 1, 2, 3), use_kv_cache=False, device_search=device_search, **opts)
        _assert_search_equals(gen._generate(sample, prefix_tokens=pre), want,
                              f"{name} {'device' if device_search else 'host'}, no cache")
