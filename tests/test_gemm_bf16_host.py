"""Host side of the bf16-operand GEMM mode of the GPT-2 decoder (no GPU): argument checks of the new entry points
before any launch, the workspace plan, the constructor and config surface, and the CPU restatement the GPU tests
lean on (tests/gpt2_bf16_ref.py): its rounding helper against torch's cast at the ties, and the restatement with
rounding switched off against tests/gpt2_dropout_ref.py."""
import ctypes

import pytest
import torch

import gpt2_bf16_ref as bref
import gpt2_dropout_ref as gref
from oracle import gpt2_ref
from vidsitu_amd import _lib

ONE = ctypes.c_void_p(16)  # a non-null pointer that is never followed: the checks come before any launch

# 1 + 2^-8 -> 1 and 1 + 2^-7 + 2^-8 -> 1 + 2^-6 (ties go to the even neighbour), their negatives, and the fp32
# neighbours either side of both ties
TIES = [1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 2.0 ** -7 + 2.0 ** -8)]
NEAR = [t + s * 2.0 ** -23 for t in TIES[:2] for s in (-1, 1)]
NEAR += [-v for v in NEAR]


def _call(x=ONE, w=ONE, y=ONE, m=4, n=4, k=4, act=0):
    lib = _lib.load()
    rc = lib.vs_gemm_nt_bf16_ws(x, w, None, None, y, m, n, k, act, None, 0, None)
    return rc, lib.vs_last_error_string()


@pytest.mark.parametrize("kw", [dict(x=None), dict(w=None), dict(y=None), dict(m=0), dict(n=0), dict(k=0), dict(m=-3),
                                dict(n=-1), dict(k=-7)], ids=str)
def test_bad_pointers_and_sizes_are_refused_before_any_launch(kw):
    rc, msg = _call(**kw)
    assert rc == -1 and b"vs_gemm_nt_bf16_ws" in msg and b"bad args" in msg


@pytest.mark.parametrize("act", [-1, 3, 100])
def test_bad_act_is_refused_with_a_message(act):
    rc, msg = _call(act=act)
    assert rc == -1 and b"vs_gemm_nt_bf16_ws" in msg and b"act must be 0 (none), 1 (relu) or 2 (gelu_new)" in msg


def test_workspace_bytes_is_zero_where_no_split_is_planned():
    ws = _lib.load().vs_gemm_nt_bf16_workspace_bytes
    # fewer than four 32-wide k-tiles per slice / one 128x128 tile per CU and more / enough 64x64 tiles already
    for shape in [(1, 1, 1), (3, 5, 7), (64, 64, 32), (65, 65, 33), (2048, 2048, 64), (2049, 2040, 72),
                  (1024, 4096, 600), (600, 8236, 1024), (600, 4096, 1024), (0, 64, 512), (64, -1, 512)]:
        assert ws(*shape) == 0, shape
    # split shapes: slices * M * N floats, with the slice count of the fp32 entry point's rule; no <= 64-row detour
    assert ws(65, 64, 512) == 4 * 65 * 64 * 4
    assert ws(65, 64, 2080) == 16 * 65 * 64 * 4
    assert ws(600, 1024, 1024) == 4 * 600 * 1024 * 4
    assert ws(600, 1024, 1024) == _lib.load().vs_gemm_nt_f32_workspace_bytes(600, 1024, 1024)
    assert ws(1, 1024, 1024) == 8 * 1024 * 4 and _lib.load().vs_gemm_nt_f32_workspace_bytes(1, 1024, 1024) == 0


def test_constructor_accepts_fp32_and_bf16_only():
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip

    assert GPT2LMHeadModelHip(1, 16, 2, 8, 11).matmul == "fp32"
    assert GPT2LMHeadModelHip(1, 16, 2, 8, 11, matmul="fp32").matmul == "fp32"
    assert GPT2LMHeadModelHip(1, 16, 2, 8, 11, matmul="bf16").matmul == "bf16"
    for bad in ("fp16", "BF16", "", None, True):
        with pytest.raises(ValueError, match="matmul"):
            GPT2LMHeadModelHip(1, 16, 2, 8, 11, matmul=bad)


def test_matmul_mode_changes_neither_names_nor_state_dict():
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip

    torch.manual_seed(0)
    a = GPT2LMHeadModelHip(1, 16, 2, 8, 11)
    torch.manual_seed(0)
    b = GPT2LMHeadModelHip(1, 16, 2, 8, 11, matmul="bf16")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    assert all(torch.equal(sa[k], sb[k]) and sa[k].dtype == torch.float32 for k in sa)


def test_config_default_is_fp32_and_the_key_can_be_overridden():
    from vidsitu_amd.extended_config import get_cfg

    assert get_cfg({}).mdl.gpt2_matmul == "fp32"
    assert get_cfg({"mdl.gpt2_matmul": "bf16"}).mdl.gpt2_matmul == "bf16"


def test_decoder_wrappers_read_the_config_key():
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    for mode in ("fp32", "bf16"):
        cfg = get_cfg({"task_type": "vb_arg", "mdl.mdl_name": "tx_only", "mdl.tx_dec_type": "gpt2",
                       "mdl.gpt2_mdl_name": "gpt2-synth-tiny", "synth.gpt2_vocab": 97, "mdl.gpt2_matmul": mode})
        mdl = get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=synth_data.make_comm(cfg))
        assert [m.matmul for m in mdl.modules() if isinstance(m, GPT2LMHeadModelHip)] == [mode]


def test_rounding_helper_is_torch_rne_at_the_ties_and_beside_them():
    v = torch.tensor(TIES + NEAR, dtype=torch.float32)
    assert v.double().tolist() == TIES + NEAR, "the probes must be exact fp32 values"
    got = bref.round_bf16(v)
    assert torch.equal(got.view(torch.int32), v.bfloat16().float().view(torch.int32))
    assert got[:4].tolist() == [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6)]
    # one ulp below / above a tie goes down / up
    assert got[4:8].tolist() == [1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -7, 1 + 2.0 ** -6]
    g = torch.Generator().manual_seed(3)
    r = torch.randn(100000, generator=g) * torch.logspace(-6, 6, 100000)
    assert torch.equal(bref.round_bf16(r).view(torch.int32), r.bfloat16().float().view(torch.int32))
    r64 = r.double()
    assert bref.round_bf16(r64).dtype == torch.float64 and torch.equal(bref.round_bf16(r64), bref.round_bf16(r).double())


def test_restatement_without_rounding_is_the_plain_restatement():
    n_layer, d, n_head, n_pos, vocab = 2, 64, 4, 64, 97
    pad = vocab - 1
    w = {k: torch.from_numpy(v) for k, v in gpt2_ref.make_weights(vocab, n_pos, d, n_layer, 23).items()}
    g = torch.Generator().manual_seed(77)
    toks = torch.randint(0, pad, (3, 23), generator=g)
    toks[1, -5:] = pad
    labels = [toks, torch.where(toks == pad, toks, torch.randint(0, pad, (3, 23), generator=g))]
    key_mask = toks.ne(pad)
    lg, ls, gr = bref.run(w, toks, key_mask, n_layer, n_head, pad, labels, torch.float64, rnd=False)
    lg0, ls0, gr0 = gref.run(w, toks, key_mask, n_layer, n_head, {}, pad, labels, torch.float64)

    def dev(a, b):
        return float((a - b).abs().max()) / float(b.abs().max())

    assert dev(lg, lg0) < 1e-13 and dev(ls, ls0) < 1e-13
    assert set(gr) == set(gr0)
    for k in gr0:
        assert dev(gr[k], gr0[k]) < 1e-12, k
    # and with rounding on it is a different function, by about bf16's 2^-9
    lgr, _, _ = bref.run(w, toks, key_mask, n_layer, n_head, pad, labels, torch.float64)
    assert 1e-4 < dev(lgr, lg0) < 3e-2
