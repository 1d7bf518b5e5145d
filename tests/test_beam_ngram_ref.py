"""n-gram blocking, the parts that need no GPU: the reference's dict of n-grams over the full row and the
kernel's scan of positions 0..step ban the same live tokens (tests/beam_ngram_ref.py), the oracle search
with the ban never repeats an n-gram, `SeqGenCustom` accepts the option, and `vs_beam_topk_ngram` checks
its arguments on the host before any launch."""
import ctypes

import numpy as np
import pytest

import beam_ngram_ref as R
from oracle import beam_ref


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_full_row_dict_and_scan_ban_the_same_live_tokens(n):
    rs = np.random.RandomState(n)
    pad, L = 1, 30
    some = 0
    for _ in range(400):
        # steps below, at and above step + 2 - n == 0, up to the last one the row has room for
        step = int(rs.randint(0, L - 1))
        row = np.full(L, pad, dtype=np.int64)
        row[: step + 1] = rs.choice([4, 5, 6, 7], size=step + 1)  # 4 values: repeats are common
        want, got = R.live(R.banned_ref(row, step, n), pad), R.live(R.banned_scan(row, step, n), pad)
        assert want == got, (row.tolist(), step, n)
        if step + 2 - n < 0:
            assert got == []
        some += len(got) > 0
        # what lies after `step` does not matter to the scan
        row[step + 1:] = rs.choice([4, 5, 6, 7], size=L - step - 1)
        assert R.live(R.banned_scan(row, step, n), pad) == got
    assert some > 40  # the comparison is not vacuous
    for step in range(0, 4):  # every step around the first one that can ban
        row = np.full(L, pad, dtype=np.int64)
        row[: step + 1] = 5
        got = R.live(R.banned_scan(row, step, n), pad)
        assert got == R.live(R.banned_ref(row, step, n), pad)
        assert (got == []) == (step + 2 - n < 0 or (n > 1 and step == n - 2))


def _stub_case(V, seed):
    table, hist, prefix = R.stub_tables(V, seed, 2)
    kw = dict(bsz=2, vocab=V, pad=1, eos=2, unk=3, beam_size=3, max_len_b=16, min_len=6, prefix_tokens=prefix)
    return R.stub_step_logits(table, hist), kw


def _tokens(fin):
    return [[h["tokens"].tolist() for h in sent] for sent in fin]


@pytest.mark.parametrize("V,seed", [(12, 2), (40, 4)])
def test_helper_without_a_ban_is_the_oracle(V, seed):
    step_logits, kw = _stub_case(V, seed)
    want = beam_ref.generate(step_logits, **kw)
    got, bans, gap = R.generate(step_logits, 0, **kw)
    assert bans == 0 and gap > 0
    assert _tokens(got) == _tokens(want)
    for sg, sw in zip(got, want):
        for hg, hw in zip(sg, sw):
            assert hg["score"] == hw["score"]
            assert np.array_equal(hg["positional_scores"], hw["positional_scores"])
    assert beam_ref.log_softmax.__module__ == "oracle.beam_ref"  # the patch is gone


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("V,seed", [(12, 2), (40, 4)])
def test_no_finalized_hypothesis_repeats_an_ngram(V, seed, n):
    step_logits, kw = _stub_case(V, seed)
    fin, bans, gap = R.generate(step_logits, n, **kw)
    assert bans >= 1
    assert _tokens(fin) != _tokens(beam_ref.generate(step_logits, **kw))
    for sent in fin:
        assert len(sent) == 3
        for h in sent:
            assert not R.has_repeated_ngram([kw["eos"]] + h["tokens"].tolist(), n)


class _Tok:
    def __len__(self):
        return 40

    def pad(self):
        return 1

    def eos(self):
        return 2

    def unk(self):
        return 3


def _stub_model():
    import torch

    class M(torch.nn.Module):
        use_encoder = False

    return M()


def test_seq_gen_accepts_the_option():
    from vidsitu_amd.seq_gen import SeqGenCustom

    gen = SeqGenCustom([_stub_model()], _Tok(), no_repeat_ngram_size=3)
    assert gen.no_repeat_ngram_size == 3
    assert SeqGenCustom([_stub_model()], _Tok()).no_repeat_ngram_size == 0
    with pytest.raises(NotImplementedError, match="no hypothesis can ever finish"):
        SeqGenCustom([_stub_model()], _Tok(), no_repeat_ngram_size=1)
    with pytest.raises(NotImplementedError):
        SeqGenCustom([_stub_model()], _Tok(), no_repeat_ngram_size=3, match_source_len=True)
    with pytest.raises(NotImplementedError):
        SeqGenCustom([_stub_model()], _Tok(), match_source_len=True)


def test_ngram_entry_point_validates_arguments_without_gpu():
    """Rejected on the host before any launch; the pointers are never dereferenced."""
    from vidsitu_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(tokens, tok_ld, step, ngram):
        return lib.vs_beam_topk_ngram(p, None, None, tokens, tok_ld, step, ngram, p, p, 1, 8, 2, 1, 2, 3,
                                      0.0, 1.0, 0, None, 0, None)

    assert call(p, 8, 0, -1) == -1
    assert b"ngram must be >= 0" in lib.vs_last_error_string()
    assert call(None, 8, 0, 2) == -1
    assert b"token history" in lib.vs_last_error_string()
    assert call(p, 8, 8, 2) == -1
    assert b"tok_ld" in lib.vs_last_error_string()
    assert call(p, 8, -1, 2) == -1
    assert b"tok_ld" in lib.vs_last_error_string()
