"""Host side of the bf16 decode step of the GPT-2 decoder (`decode_matmul="bf16"`, no GPU): argument checks of
vs_pack_rows_bf16 / vs_gemm_nt_bf16_packed before any launch, the tile-shape query against the entry point's refusals
and against the GPU test's shape list, the bf16 weight image's layout stated a second time in index arithmetic, and
the constructor / config surface."""
import ctypes

import pytest
import torch

from test_gemm_bf16_host import NEAR, TIES
from test_gpu_gpt2_decode_bf16 import CASES
from vidsitu_amd import _lib, ops

ONE = ctypes.c_void_p(16)  # a non-null, 16-byte aligned pointer that is never followed: every call here is refused


def _gemm(x=ONE, w=ONE, y=ONE, m=4, n=16, k=128, act=0, ypk=0):
    lib = _lib.load()
    rc = lib.vs_gemm_nt_bf16_packed(x, w, None, None, y, m, n, k, act, ypk, None)
    return rc, lib.vs_last_error_string()


def _pack(src=ONE, dst=ONE, r=4, k=32):
    lib = _lib.load()
    rc = lib.vs_pack_rows_bf16(src, dst, r, k, None)
    return rc, lib.vs_last_error_string()


@pytest.mark.parametrize("kw", [dict(x=None), dict(w=None), dict(y=None), dict(m=0), dict(m=65), dict(m=-1), dict(n=0),
                                dict(k=0), dict(n=-5)], ids=str)
def test_gemm_bad_pointers_and_row_counts_are_refused_before_any_launch(kw):
    rc, msg = _gemm(**kw)
    assert rc == -1 and b"vs_gemm_nt_bf16_packed" in msg and b"1..64 rows" in msg


@pytest.mark.parametrize("k", [1, 32, 64, 96, 127, 129, 160, 192, 1000])
def test_gemm_k_off_the_128_grid_is_refused(k):
    rc, msg = _gemm(k=k)
    assert rc == -1 and b"vs_gemm_nt_bf16_packed" in msg and b"K must be a multiple of 128" in msg


@pytest.mark.parametrize("act", [-1, 3, 100])
def test_gemm_bad_act_is_refused(act):
    rc, msg = _gemm(act=act)
    assert rc == -1 and b"vs_gemm_nt_bf16_packed" in msg and b"act must be 0 (none), 1 (relu) or 2 (gelu_new)" in msg


@pytest.mark.parametrize("n", [1, 15, 17, 97])
def test_gemm_packed_output_needs_whole_column_blocks(n):
    rc, msg = _gemm(n=n, ypk=1)
    assert rc == -1 and b"vs_gemm_nt_bf16_packed" in msg and b"a packed output needs N % 16 == 0" in msg


@pytest.mark.parametrize("kw", [dict(x=ctypes.c_void_p(20)), dict(w=ctypes.c_void_p(18))], ids=["x", "w"])
def test_gemm_unaligned_operands_are_refused(kw):
    rc, msg = _gemm(**kw)
    assert rc == -1 and b"vs_gemm_nt_bf16_packed" in msg and b"unaligned operands" in msg


@pytest.mark.parametrize("kw", [dict(src=None), dict(dst=None), dict(r=0), dict(r=-2), dict(k=0), dict(k=16), dict(k=48),
                                dict(k=33), dict(k=-32)], ids=str)
def test_pack_bad_arguments_are_refused_before_any_launch(kw):
    rc, msg = _pack(**kw)
    assert rc == -1 and b"vs_pack_rows_bf16" in msg and b"K must be a multiple of 32" in msg


@pytest.mark.parametrize("kw", [dict(src=ctypes.c_void_p(24)), dict(dst=ctypes.c_void_p(8))], ids=["src", "dst"])
def test_pack_unaligned_pointers_are_refused(kw):
    rc, msg = _pack(**kw)
    assert rc == -1 and b"vs_pack_rows_bf16" in msg and b"16-byte aligned pointers" in msg


def test_plan_is_minus_one_exactly_where_the_entry_point_refuses():
    """The entry point takes 1 <= M <= 64, N >= 1, K a positive multiple of 128 (its header comment): the query says
    -1 on every other triple, and on those the entry point itself refuses (it is called only there: a taken triple
    would launch)."""
    lib = _lib.load()
    count = lib.vs_gemm_nt_bf16_packed_plan_count()
    assert count >= 1
    for m in (-1, 0, 1, 16, 17, 64, 65, 1000):
        for n in (-1, 0, 1, 16, 97, 3039, 3040, 12159, 12160, 50259):
            for k in (-128, 0, 32, 64, 127, 128, 160, 256, 384, 1000, 1024, 4096):
                plan = lib.vs_gemm_nt_bf16_packed_plan(m, n, k)
                taken = 1 <= m <= 64 and n >= 1 and k >= 1 and k % 128 == 0
                assert (plan >= 0) == taken and -1 <= plan < count, (m, n, k, plan)
                if not taken:
                    assert _gemm(m=m, n=n, k=k)[0] == -1, (m, n, k)


def test_gpu_shape_list_takes_every_plan():
    lib = _lib.load()
    plans = {lib.vs_gemm_nt_bf16_packed_plan(c[0], c[1], c[2]) for c in CASES}
    assert plans == set(range(lib.vs_gemm_nt_bf16_packed_plan_count())), sorted(plans)


# ---------------------------------------------------------------------------------------------
# the weight image, stated in index arithmetic
# ---------------------------------------------------------------------------------------------
def _pack_restated(w):
    """Element (r, k) of w, rounded to bf16, goes to block (r // 16) * (K // 32) + k // 32 (512 values each), lane
    (k % 32 // 8) * 16 + r % 16 (8 values each), slot k % 8; what no element reaches is zero."""
    rows, kk = w.shape
    r = torch.arange(rows).view(-1, 1).expand(rows, kk)
    k = torch.arange(kk).view(1, -1).expand(rows, kk)
    pos = ((r // 16) * (kk // 32) + k // 32) * 512 + ((k % 32 // 8) * 16 + r % 16) * 8 + k % 8
    assert pos.unique().numel() == rows * kk
    out = torch.zeros((rows + 15) // 16 * 16 * kk, dtype=torch.bfloat16)
    out[pos.reshape(-1)] = w.bfloat16().reshape(-1)
    return out.view(torch.int16)


@pytest.mark.parametrize("k", [32, 128, 160])
@pytest.mark.parametrize("rows", [1, 16, 17, 50])
def test_unpack_inverts_the_restated_image(rows, k):
    g = torch.Generator().manual_seed(rows * 1000 + k)
    w = torch.randn(rows, k, generator=g) * torch.logspace(-3, 3, k)
    probes = torch.tensor(TIES + NEAR, dtype=torch.float32)
    w.view(-1)[: probes.numel()] = probes  # (rows * k >= 32 > 12)
    img = _pack_restated(w)
    assert img.numel() == (rows + 15) // 16 * 16 * k
    back = ops.unpack_rows_bf16(img, rows, k)
    assert back.dtype == torch.float32 and tuple(back.shape) == (rows, k)
    assert torch.equal(back.view(torch.int32), w.bfloat16().float().view(torch.int32))
    # the ties go to the even neighbour, one ulp beside a tie goes to the nearer one
    assert back.view(-1)[:4].tolist() == [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6)]
    assert back.view(-1)[4:8].tolist() == [1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -7, 1 + 2.0 ** -6]
    # the zero-filled rows, read back as rows of a 16-row multiple
    full = ops.unpack_rows_bf16(img, (rows + 15) // 16 * 16, k)
    assert torch.equal(full[:rows], back) and not bool(full[rows:].any())


# ---------------------------------------------------------------------------------------------
# constructor and config
# ---------------------------------------------------------------------------------------------
def test_constructor_accepts_fp32_and_bf16_only():
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip

    assert GPT2LMHeadModelHip(1, 16, 2, 8, 11).decode_matmul == "fp32"
    assert GPT2LMHeadModelHip(1, 16, 2, 8, 11, decode_matmul="fp32").decode_matmul == "fp32"
    m = GPT2LMHeadModelHip(1, 16, 2, 8, 11, decode_matmul="bf16")
    assert m.decode_matmul == "bf16" and m.matmul == "fp32"  # the two switches are separate
    assert GPT2LMHeadModelHip(1, 16, 2, 8, 11, matmul="bf16").decode_matmul == "fp32"
    for bad in ("fp16", "BF16", "", None, True):
        with pytest.raises(ValueError, match="decode_matmul"):
            GPT2LMHeadModelHip(1, 16, 2, 8, 11, decode_matmul=bad)


def test_mode_changes_neither_names_nor_state_dict_and_has_a_cache_of_its_own():
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip

    torch.manual_seed(0)
    a = GPT2LMHeadModelHip(1, 16, 2, 8, 11)
    torch.manual_seed(0)
    b = GPT2LMHeadModelHip(1, 16, 2, 8, 11, decode_matmul="bf16")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) and sa[k].dtype == torch.float32 for k in sa)
    assert "_wpk16" in GPT2LMHeadModelHip._CACHES and b._wpk16 == {}
    b._wpk16["k"] = torch.zeros(1)
    b.load_state_dict(sa)  # a load drops the derived copies, the bf16 images among them
    assert b._wpk16 == {}


def test_config_default_is_fp32_and_the_key_can_be_overridden():
    from vidsitu_amd.extended_config import get_cfg

    assert get_cfg({}).mdl.gpt2_decode_matmul == "fp32"
    cfg = get_cfg({"mdl.gpt2_decode_matmul": "bf16"})
    assert cfg.mdl.gpt2_decode_matmul == "bf16" and cfg.mdl.gpt2_matmul == "fp32"


@pytest.mark.parametrize("mdl_name", ["tx_only", "new_gpt2_only"])
def test_both_construction_sites_read_the_config_key(mdl_name):
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    for mode in ("fp32", "bf16"):
        cfg = get_cfg({"task_type": "vb_arg", "mdl.mdl_name": mdl_name, "mdl.tx_dec_type": "gpt2",
                       "mdl.gpt2_mdl_name": "gpt2-synth-tiny", "synth.gpt2_vocab": 97, "mdl.gpt2_decode_matmul": mode})
        mdl = get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=synth_data.make_comm(cfg))
        got = [(m.decode_matmul, m.matmul) for m in mdl.modules() if isinstance(m, GPT2LMHeadModelHip)]
        assert got == [(mode, "fp32")]
