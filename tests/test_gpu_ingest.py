"""Fused frame ingest (`vs_ingest_u8`): one launch from decoded uint8 frames to both pathways' packed stem inputs,
bit for bit the four-launch chain (`resize_bicubic_u8` -> `frames_u8_pack` per pathway) and bit for bit a CPU
composition that uses none of the project's kernels (the resize oracle per frame, `reference_tensors`' operation order,
one bf16 rounding); and the model-level wiring: an eval forward on `frms_ev_raw_u8` is ONE ingest launch, a
training-mode forward keeps the chain, the logits are those of the host-resized `frms_ev_fast_u8` batch."""
import itertools

import numpy as np
import pytest
import torch

from oracle import resize_ref

pytestmark = pytest.mark.gpu

MEAN, STD = (0.45, 0.40, 0.50), (0.225, 0.25, 0.2)
SIZES = [((360, 640), (224, 224)), ((256, 340), (224, 224)), ((240, 320), (224, 224)), ((224, 398), (224, 224)),
         ((100, 224), (224, 224)), ((1080, 1920), (224, 224)), ((224, 224), (224, 224)), ((45, 80), (64, 64)),
         ((33, 47), (64, 16))]
ALPHA = 4


def _bits(act):
    """bf16 activation [N, C, T, H, W] (channels-last memory) -> int16 [N, T, H, W, C] of its bit patterns."""
    return act.permute(0, 2, 3, 4, 1).contiguous().view(torch.int16)


def _nan_act(ops, n, c, t, h, w, dev):
    y = ops.new_act(n, c, t, h, w, dev)
    y.view(torch.int16).fill_(0x7FC1)  # a NaN: an element the kernel leaves alone cannot equal anything
    return y


def _slow_idx(t, dev):
    return torch.linspace(0, t - 1, t // ALPHA).long().to(torch.int32).to(dev)


def _cpu_reference(frames, out_hw, cpad, reverse, tidx):
    """uint8 [N, T, H0, W0, 3] numpy -> (fast, slow) int16 bit patterns [N, T', Ho, Wo, cpad], no project kernel."""
    n, t = frames.shape[:2]
    res = np.stack([resize_ref.resize_bicubic_u8(f, *out_hw) for f in frames.reshape((-1,) + frames.shape[2:])])
    x = torch.from_numpy(res).view(n, t, out_hw[0], out_hw[1], 3)
    if reverse:
        x = x.flip(-1)
    x = x.float() / 255.0  # synth_data.reference_tensors: tensor_normalize's order
    x = x - torch.tensor(MEAN)
    x = x / torch.tensor(STD)
    full = torch.zeros(n, t, out_hw[0], out_hw[1], cpad, dtype=torch.bfloat16)
    full[..., :3] = x.to(torch.bfloat16)
    fast = full.view(torch.int16)
    slow = None if tidx is None else full.index_select(1, tidx.cpu().long()).contiguous().view(torch.int16)
    return fast, slow


@pytest.mark.parametrize("src_hw,out_hw", SIZES, ids=[f"{s[0]}x{s[1]}to{o[0]}x{o[1]}" for s, o in SIZES])
def test_ingest_is_bitwise_the_chain_and_the_cpu_composition(src_hw, out_hw, dev):
    from vidsitu_amd import ops

    big = src_hw == (1080, 1920)
    oracle_done = False
    for n, t in ([(1, 8)] if big else [(1, 8), (1, 32), (3, 8), (3, 32)]):
        g = torch.Generator().manual_seed(1000 * n + t + src_hw[0])
        frames = torch.randint(0, 256, (n, t) + src_hw + (3,), generator=g, dtype=torch.int32).to(torch.uint8)
        fr = frames.to(dev)
        resized = ops.resize_bicubic_u8(fr, *out_hw)  # the parent's chain, first half (two launches)
        for cpad, reverse, with_slow in itertools.product((4, 8), (False, True), (True, False)):
            tidx = _slow_idx(t, dev) if with_slow else None
            want_f = _bits(ops.frames_u8_pack(resized, cpad, None, MEAN, STD, reverse))
            want_s = _bits(ops.frames_u8_pack(resized, cpad, tidx, MEAN, STD, reverse)) if with_slow else None
            out_f = _nan_act(ops, n, cpad, t, out_hw[0], out_hw[1], dev)
            out_s = _nan_act(ops, n, cpad, t // ALPHA, out_hw[0], out_hw[1], dev) if with_slow else None
            got_f, got_s = ops.ingest_u8(fr, out_hw[0], out_hw[1], cpad, tidx, cpad, MEAN, STD, reverse,
                                         out=(out_f, out_s))
            what = (src_hw, out_hw, n, t, cpad, reverse, with_slow)
            assert got_f is out_f and got_s is out_s
            assert torch.equal(_bits(got_f), want_f), what
            if with_slow:
                assert torch.equal(_bits(got_s), want_s), what
            if not oracle_done and with_slow:  # once per source size: the oracle is slow
                ref_f, ref_s = _cpu_reference(frames.numpy(), out_hw, cpad, reverse, tidx)
                assert torch.equal(_bits(got_f).cpu(), ref_f), what
                assert torch.equal(_bits(got_s).cpu(), ref_s), what
                oracle_done = True
    assert oracle_done


def test_ingest_mixed_pack_widths_and_allocating_form(dev):
    """The two pathways may take different packed widths (a stem kernel beside a generic one); without `out` the
    wrapper allocates."""
    from vidsitu_amd import ops

    fr = torch.randint(0, 256, (2, 8, 45, 80, 3), generator=torch.Generator().manual_seed(5)).to(torch.uint8).to(dev)
    tidx = _slow_idx(8, dev)
    res = ops.resize_bicubic_u8(fr, 64, 64)
    got_f, got_s = ops.ingest_u8(fr, 64, 64, 4, tidx, 8, MEAN, STD)
    assert torch.equal(_bits(got_f), _bits(ops.frames_u8_pack(res, 4, None, MEAN, STD)))
    assert torch.equal(_bits(got_s), _bits(ops.frames_u8_pack(res, 8, tidx, MEAN, STD)))
    rep = torch.tensor([0, 3, 3, 7, 0], dtype=torch.int32, device=dev)  # an index may name a frame more than once
    got_f, got_s = ops.ingest_u8(fr, 64, 64, 8, rep, 4, MEAN, STD, True)
    assert torch.equal(_bits(got_s), _bits(ops.frames_u8_pack(res, 4, rep, MEAN, STD, True)))
    got_f, got_s = ops.ingest_u8(fr, 64, 64, 8)
    assert got_s is None
    assert torch.equal(_bits(got_f), _bits(ops.frames_u8_pack(res, 8)))


@pytest.mark.parametrize("name", ["slow_fast_mini", "i3d_tiny"])
def test_eval_forward_on_raw_frames_is_one_ingest_launch(name, dev, monkeypatch):
    from vidsitu_amd import _lib, synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    cfg = get_cfg({"mdl.sf_mdl_name": name, "synth.num_verbs": 23})
    crop = int(cfg.sf_mdl.DATA.TRAIN_CROP_SIZE)
    comm = synth_data.make_comm(cfg)
    torch.manual_seed(0)
    mdl = get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=comm).to(dev).eval()
    t = cfg.sf_mdl.DATA.NUM_FRAMES
    raw = torch.randint(0, 256, (1, 2, t, 45, 80, 3), generator=torch.Generator().manual_seed(1)).to(torch.uint8)
    host = np.stack([resize_ref.resize_bicubic_u8(f, crop, crop) for f in raw.reshape(-1, 45, 80, 3).numpy()])
    host = torch.from_numpy(host).view(1, 2, t, crop, crop, 3)
    common = {"vseg_idx": torch.arange(1, device=dev)}

    names = []
    real_call = _lib.call

    def recording_call(entry, *args):
        names.append(entry)
        return real_call(entry, *args)

    monkeypatch.setattr(_lib, "call", recording_call)
    with torch.no_grad():
        a = mdl({"frms_ev_raw_u8": raw.to(dev), **common})["mdl_out"]
    assert names.count("vs_ingest_u8") == 1
    assert "vs_resize_bicubic_u8" not in names and "vs_frames_u8_pack" not in names
    names.clear()
    with torch.no_grad():
        b = mdl({"frms_ev_fast_u8": host.to(dev), **common})["mdl_out"]
    assert "vs_ingest_u8" not in names
    assert torch.equal(a, b)

    names.clear()
    mdl.train()
    mdl({"frms_ev_raw_u8": raw.to(dev), **common})
    assert "vs_ingest_u8" not in names
    assert names.count("vs_resize_bicubic_u8") == 1
    assert names.count("vs_frames_u8_pack") == mdl.sf_mdl.num_pathways
