"""The dropout generator contract without a GPU: known answers of Philox4x32-10, the library's host-side mask
(`vs_dropout_mask_host`, the same inline the kernels use) against the numpy restatement of tests/dropout_ref.py bit
for bit, the statistics the contract promises (checked on the restatement, which the library equals), the refused
probabilities, and the config key."""
import ctypes
import math
import os

import numpy as np
import pytest

import dropout_ref as ref
from vidsitu_amd import _lib, ops
from vidsitu_amd.extended_config import get_cfg

REF_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_vsitu_cfg.yml")

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
PS = [0.0, 0.1, 0.5, 0.9]
BIG_SEED = (0x1234 << 32) | 0x9abcdef1  # above 2^32: both key words are in play
BIG_E0 = (1 << 34) + 5  # above 2^34: the high word of the block counter is non-zero
N_STAT = 1 << 16
STAT_SEED, STAT_STEP, STAT_SITE = 20240607, 3, 4


def _lib_words(ctr, key):
    """The library's Philox block for an arbitrary counter / key, read through the mask with thr = word + 0 / + 1:
    counter = (b lo, b hi, site, step), key = (seed lo, seed hi)."""
    seed, step, site, b = key[0] | (key[1] << 32), ctr[3], ctr[2], ctr[0] | (ctr[1] << 32)
    want = ref.philox4x32_10(ctr, key)
    for k in range(4):  # keep iff word >= thr: true at thr = word, false at thr = word + 1
        w = int(want[k])
        assert ops.dropout_mask_host(seed, step, site, 4 * b + k, 1, w).tolist() == [1]
        if w < 0xffffffff:
            assert ops.dropout_mask_host(seed, step, site, 4 * b + k, 1, w + 1).tolist() == [0]
    return want


@pytest.mark.parametrize("ctr,key,out", KNOWN_ANSWERS)
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(x) for x in ref.philox4x32_10(ctr, key)) == out
    # the library's generator produces the same words (b = 2^64 - 1 would overflow 4b + k: the all-ones vector is
    # checked on the restatement only)
    if ctr[1] < 1 << 30:
        assert tuple(int(x) for x in _lib_words(ctr, key)) == out


def test_threshold_follows_the_contract():
    for p in PS + [0.25, 1e-10, 1.0 - 1e-12]:
        thr, scale = ops.dropout_params(p)
        assert (thr, scale) == ref.threshold(p), p
        assert thr == min(int(math.floor(p * 2.0 ** 32 + 0.5)), 0xffffffff)
    assert ops.dropout_params(0.0) == (0, 1.0)


@pytest.mark.parametrize("p", [-0.1, -1e-9, 1.0, 1.5, float("nan")])
def test_probability_out_of_range_is_refused(p):
    lib = _lib.load()
    thr, scale = ctypes.c_uint32(77), ctypes.c_float(77.0)
    assert lib.vs_dropout_threshold(p, ctypes.byref(thr), ctypes.byref(scale)) == -1  # VS_ERR_BAD_ARG
    assert b"0 <= p < 1" in lib.vs_last_error_string()
    assert (thr.value, scale.value) == (77, 77.0)
    with pytest.raises(_lib.VsError):
        ops.dropout_params(p)
    # the model refuses it at construction, before any launch
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip
    with pytest.raises(_lib.VsError):
        GPT2LMHeadModelHip(1, 16, 2, 8, 11, attn_pdrop=p)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("e0", [0, 1, 5, BIG_E0])
def test_host_mask_equals_the_restatement(e0, p):
    thr, _ = ref.threshold(p)
    for n in (1, 3, 4, 1025):
        for seed, step, site in ((7, 0, 0), (BIG_SEED, 3, 1), (BIG_SEED, (1 << 32) + 9, 73), (2 ** 63 + 11, 5, 2)):
            got = ops.dropout_mask_host(seed, step, site, e0, n, thr).numpy()
            want = ref.keep_flat(seed, step, site, n, thr, e0)
            assert np.array_equal(got, want), (e0, n, p, seed, step, site)
            if p == 0.0:
                assert got.all(), "p = 0 keeps everything"


def test_step_uses_its_low_32_bits_and_the_seed_all_64():
    thr, _ = ref.threshold(0.5)
    a = ops.dropout_mask_host(BIG_SEED, 9, 1, 0, 256, thr)
    assert a.tolist() == ops.dropout_mask_host(BIG_SEED, (1 << 32) + 9, 1, 0, 256, thr).tolist()
    assert a.tolist() != ops.dropout_mask_host(BIG_SEED & 0xffffffff, 9, 1, 0, 256, thr).tolist()


def _sigma_share(p):
    return math.sqrt(p * (1.0 - p) / N_STAT)


@pytest.mark.parametrize("p", PS[1:])
def test_kept_share(p):
    thr, _ = ref.threshold(p)
    want = ref.keep_flat(STAT_SEED, STAT_STEP, STAT_SITE, N_STAT, thr)
    share = float(want.mean())
    print(f"DROPOUT kept share p={p}: {share:.5f} vs {1 - p:.5f}, 5 sigma = {5 * _sigma_share(p):.5f}")
    assert abs(share - (1.0 - p)) <= 5.0 * _sigma_share(p)  # a condition on the restatement ...
    got = ops.dropout_mask_host(STAT_SEED, STAT_STEP, STAT_SITE, 0, N_STAT, thr).numpy()
    assert np.array_equal(got, want)  # ... which the library equals


@pytest.mark.parametrize("p", PS[1:])
@pytest.mark.parametrize("what", ["site", "step", "seed"])
def test_masks_of_different_sites_steps_seeds_are_independent(what, p):
    """Two independent masks agree on a share q = (1-p)^2 + p^2 of the elements; sigma = sqrt(q (1-q) / n)."""
    thr, _ = ref.threshold(p)
    other = {"site": (STAT_SEED, STAT_STEP, STAT_SITE + 1), "step": (STAT_SEED, STAT_STEP + 1, STAT_SITE),
             "seed": (STAT_SEED + 1, STAT_STEP, STAT_SITE)}[what]
    a = ref.keep_flat(STAT_SEED, STAT_STEP, STAT_SITE, N_STAT, thr)
    b = ref.keep_flat(*other, N_STAT, thr)
    q = (1.0 - p) ** 2 + p ** 2
    agree = float((a == b).mean())
    sigma = math.sqrt(q * (1.0 - q) / N_STAT)
    print(f"DROPOUT agreement p={p} other {what}: {agree:.5f} vs {q:.5f}, 5 sigma = {5 * sigma:.5f}")
    assert abs(agree - q) <= 5.0 * sigma
    assert np.array_equal(ops.dropout_mask_host(*other, 0, N_STAT, thr).numpy(), b)


def test_attention_index_puts_four_keys_of_a_query_in_one_block():
    """The padded pitch of the attention site: keep_attn's element of (r, h, i, j) is ((r*H + h)*L + i)*Lp + j."""
    r, h, l, thr = 2, 3, 5, ref.threshold(0.5)[0]
    m = ref.keep_attn(11, 2, 4, r, h, l, thr)
    assert m.shape == (r, h, l, l)
    lp = 8
    for (ri, hi, i, j) in ((0, 0, 0, 0), (1, 2, 4, 4), (0, 1, 3, 2)):
        e = ((ri * h + hi) * l + i) * lp + j
        assert int(m[ri, hi, i, j]) == int(ops.dropout_mask_host(11, 2, 4, e, 1, thr)[0])


def test_config_key_defaults_to_zero():
    assert get_cfg().mdl.gpt2_dropout == 0.0
    assert get_cfg(cfg_pth=REF_CFG).mdl.gpt2_dropout == 0.0  # the reference's own file does not carry the key
    assert get_cfg({"mdl.gpt2_dropout": 0.1}, cfg_pth=REF_CFG).mdl.gpt2_dropout == 0.1
    assert get_cfg({"mdl.gpt2_dropout": 0.1}).mdl.gpt2_dropout == 0.1


def test_state_must_exist_before_a_capture_and_survives_a_device_move(monkeypatch):
    """Host logic of the model's [seed, step] state (a capture is answered here, as tests/test_flat_module.py does):
    created at the first train-mode forward from torch's default CPU generator, refused inside a capture, not part
    of the state dict, set and read back, kept across `.to()`."""
    import torch

    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip

    m = GPT2LMHeadModelHip(1, 16, 2, 8, 11, resid_pdrop=0.1)
    assert m.dropout_state() is None and m._dropout_on()
    assert not GPT2LMHeadModelHip(1, 16, 2, 8, 11)._dropout_on()
    keys = set(m.state_dict())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.VsError, match="dropout state must exist before a graph capture"):
        m._drop_state_on(torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    torch.manual_seed(123)
    st = m._drop_state_on(torch.device("cpu"))
    torch.manual_seed(123)
    assert st.tolist() == [int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)), 0]
    assert m._drop_state_on(torch.device("cpu")) is st
    m.set_dropout_state((BIG_SEED, 17))
    assert m._drop_state is st and m.dropout_state() == (BIG_SEED, 17)  # written in place: graphs keep their memory
    m = m.to(torch.float64).to("cpu")
    assert m.dropout_state() == (BIG_SEED, 17) and m._drop_state.dtype == torch.int64
    assert set(m.state_dict()) == keys and not list(m.buffers())
