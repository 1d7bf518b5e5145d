"""The key-tiled attention family (csrc/attn_tiled.hip) through its own entry points, at small L: both sides of the
64-query and 64-key tile edges, one to four key tiles, both masking rules, both dropout modes.

Tolerance: the project's rule for fp32 kernels, unchanged (tests/test_gpu_roberta_ops.py, tests/test_gpu_gpt2_ops.py):
the kernel's error against fp64, max |diff| / max |fp64|, is at most 16 x the fp32 CPU restatement's own error and never
above 2e-4; a quantity that is exactly zero in fp64 is exactly zero.  Causal queries in front of left padding (every
visible key masked) are held as tests/test_gpu_gpt2_ops.py holds them: FULLY_MASKED_BOUND of max |v| against the
reference with fp32-formed scores.  References: roberta_ref.attention / roberta_dropout_ref.attention (padding rule),
the _attn_ref construction of tests/test_gpu_gpt2_ops.py / gpt2_dropout_ref.attention (causal rule) -- the cases, their
inputs and their references are those modules' cached ones.  docs/roberta_ops_parity.md and docs/gpt2_ops_parity.md
hold the measured tables.  Every figure is printed (`PARITY ...`) before it is asserted.
"""
import pytest
import torch

import test_gpu_gpt2_dropout as gd
import test_gpu_gpt2_ops as go
import test_gpu_roberta_dropout as rd
import test_gpu_roberta_ops as ro

pytestmark = pytest.mark.gpu

NAN = float("nan")
R = 3
LS = [1, 15, 17, 63, 64, 65, 127, 129, 200]
# (H, dh): H in {1, 3} x dh in {32, 64}, one case each at dh = 16 and dh = 128
HEADS = [(1, 32), (3, 32), (1, 64), (3, 64)]
SHAPES = [(l, h, dh) for l in LS for h, dh in HEADS] + [(129, 3, 16), (65, 1, 128)]
SHAPE_IDS = [f"L{l}_H{h}_dh{dh}" for l, h, dh in SHAPES]
CAUSAL_MASKS = ("none", "right", "left")


def _fwd(ops, qkv, mask, r, l, h, dh, causal, drop=None, out=None):
    out = torch.full((r * l, h * dh), NAN, device=qkv.device) if out is None else out
    snap, site, thr, scale = (None, 0, 0, 1.0) if drop is None else drop
    ops._lib.call("vs_attn_tiled_fwd", ops._ptr(qkv), ops._ptr(mask), ops._ptr(out), r, l, h, dh, int(causal),
                  ops._ptr(snap), site, thr, scale, ops._stream())
    return out


def _bwd(ops, qkv, mask, dout, r, l, h, dh, causal, drop=None):
    """Into NaN-filled dqkv with the whole scratch workspace full of NaN: every output has an owner, no stale scratch
    is read."""
    need = ops._lib.load().vs_attn_tiled_bwd_scratch_bytes(r, l, h)
    assert need == r * h * 3 * l * 4, "the scratch is three [R*H][L] rows of floats, never an L x L matrix"
    ws = ops._workspace(need, qkv.device)
    ws.view(torch.float32).fill_(NAN)
    dqkv = torch.full_like(qkv, NAN)
    snap, site, thr, scale = (None, 0, 0, 1.0) if drop is None else drop
    ops._lib.call("vs_attn_tiled_bwd", ops._ptr(qkv), ops._ptr(mask), ops._ptr(dout), ops._ptr(dqkv), ops._ptr(ws),
                  ws.numel(), r, l, h, dh, int(causal), ops._ptr(snap), site, thr, scale, ops._stream())
    return dqkv


def _parts(name, check, dqkv, g64, g32, d):
    assert bool(torch.isfinite(dqkv).all()), name + ": an element of dqkv has no owner, or NaN scratch / LDS was read"
    for i, part in enumerate(("dq", "dk", "dv")):
        sl = slice(i * d, (i + 1) * d)
        check(f"{name} {part}", dqkv[:, sl], g64[:, sl], g32[:, sl])


# ---------------------------------------------------------------------------------------------
# padding rule
# ---------------------------------------------------------------------------------------------
def _pad_case(ops, dev, r, l, h, dh, kind):
    c = ro._attn_case(r, l, h, dh, kind)
    mask_d = None if c["mask"] is None else c["mask"].to(torch.uint8).to(dev)
    return c, c["qkv"].to(dev), c["dout"].to(dev), mask_d


def _pad_plain(ops, dev, r, l, h, dh):
    d = h * dh
    for kind in ro.MASKS:
        c, qkv_d, dout_d, mask_d = _pad_case(ops, dev, r, l, h, dh, kind)
        name = f"attn_tiled pad R{r} L{l} H{h} dh{dh} {kind}"
        out = _fwd(ops, qkv_d, mask_d, r, l, h, dh, False)
        ro._check(name + " fwd", out, c["o64"], c["o32"])
        assert torch.equal(out, _fwd(ops, qkv_d, mask_d, r, l, h, dh, False)), name + ": forward runs differ"
        dqkv = _bwd(ops, qkv_d, mask_d, dout_d, r, l, h, dh, False)
        _parts(name, ro._check, dqkv, c["g64"], c["g32"], d)
        assert torch.equal(dqkv, _bwd(ops, qkv_d, mask_d, dout_d, r, l, h, dh, False)), name + ": backward runs differ"


@pytest.mark.parametrize("l,h,dh", SHAPES, ids=SHAPE_IDS)
def test_pad_fwd_bwd(l, h, dh, dev):
    """Every mask kind (none, right padding down to one valid key, left padding, a sequence whose mask is all zero)."""
    from vidsitu_amd import ops

    _pad_plain(ops, dev, R, l, h, dh)


def test_pad_the_shape_the_resident_kernel_refuses(dev):
    """(R, L, H, dh) = (1, 200, 2, 128): tests/test_gpu_roberta_ops.py pins the resident kernel to refuse it."""
    from vidsitu_amd import ops

    assert ops._lib.load().vs_attn_resident_fits(0, 200, 128, 0) == 0
    _pad_plain(ops, dev, 1, 200, 2, 128)


# ---------------------------------------------------------------------------------------------
# causal rule
# ---------------------------------------------------------------------------------------------
def _causal_fwd_check(name, out, c, vmax):
    ok, fm = ~c["fm"], c["fm"]
    assert bool(torch.isfinite(out).all()), name
    if bool(ok.any()):
        go._check(name, out[ok.to(out.device)], c["out64"][ok], c["out32"][ok])
    if bool(fm.any()):  # fully masked queries: future keys take softmax weight; fp32-formed scores in the reference
        err = float((out[fm.to(out.device)].cpu().double() - c["out64"][fm]).abs().max()) / vmax
        print(f"PARITY {name} [fully masked queries, of max|v|] bound={go.FULLY_MASKED_BOUND:.1e} err={err:.3e}")
        assert err <= go.FULLY_MASKED_BOUND


@pytest.mark.parametrize("l,h,dh", SHAPES, ids=SHAPE_IDS)
def test_causal_fwd_bwd(l, h, dh, dev):
    """none / right / left padding; fully masked queries (in front of left padding, or a sequence the mask empties)
    carry no loss here, the rows around them hold the normal bound."""
    from vidsitu_amd import ops

    d = h * dh
    for kind in CAUSAL_MASKS:
        c = go._attn_case(R, l, h, dh, kind)
        name = f"attn_tiled causal R{R} L{l} H{h} dh{dh} {kind}"
        qkv_d, dout_d = c["qkv"].to(dev), c["dout"].to(dev)
        mask_d = None if c["mask"] is None else c["mask"].to(dev)
        out = _fwd(ops, qkv_d, mask_d, R, l, h, dh, True)
        _causal_fwd_check(name + " fwd", out, c, float(c["qkv"][:, 2 * d:].abs().max()))
        assert torch.equal(out, _fwd(ops, qkv_d, mask_d, R, l, h, dh, True)), name + ": forward runs differ"
        dqkv = _bwd(ops, qkv_d, mask_d, dout_d, R, l, h, dh, True)
        _parts(name, go._check, dqkv, c["g64"], c["g32"], d)
        assert torch.equal(dqkv, _bwd(ops, qkv_d, mask_d, dout_d, R, l, h, dh, True)), name + ": backward runs differ"


@pytest.mark.parametrize("l,h,dh", SHAPES, ids=SHAPE_IDS)
def test_causal_loss_on_fully_masked_queries(l, h, dh, dev):
    """left_small (one pad in front of row 0, three in front of row 1) with a gradient on the fully masked queries: the
    only place where a future key j > i has dS_ij != 0 -- dV_j takes it, dK_j and dQ_i do not -- and where a tile above
    the diagonal may not be skipped.  Bound as test_attn_causal_bwd_loss_on_fully_masked_queries: nm = 3 such queries
    at most add into one element, each good to FULLY_MASKED_BOUND of the slice's largest."""
    from vidsitu_amd import ops

    r, nm, d = 2, 3, h * dh
    c = go._attn_case(r, l, h, dh, "left_small", True)
    name = f"attn_tiled causal R{r} L{l} H{h} dh{dh} left_small+loss"
    qkv_d, dout_d, mask_d = c["qkv"].to(dev), c["dout"].to(dev), c["mask"].to(dev)
    out = _fwd(ops, qkv_d, mask_d, r, l, h, dh, True)
    _causal_fwd_check(name + " fwd", out, c, float(c["qkv"][:, 2 * d:].abs().max()))
    dqkv = _bwd(ops, qkv_d, mask_d, dout_d, r, l, h, dh, True)
    assert bool(torch.isfinite(dqkv).all())
    for i, part in enumerate(("dq", "dk", "dv")):
        sl = slice(i * d, (i + 1) * d)
        ref = c["g64"][:, sl]
        top = float(ref.abs().max())
        diff = float((dqkv[:, sl].cpu().double() - ref).abs().max())
        if top == 0.0:  # (L = 1: one key, p = 1)
            print(f"PARITY {name} {part} fp64 value is exactly zero, max |got| = {diff:.3e}")
            assert diff == 0.0
            continue
        print(f"PARITY {name} {part} bound={nm * go.FULLY_MASKED_BOUND:.1e} err={diff / top:.3e}")
        assert diff / top <= nm * go.FULLY_MASKED_BOUND, part
    assert torch.equal(dqkv, _bwd(ops, qkv_d, mask_d, dout_d, r, l, h, dh, True)), name + ": backward runs differ"


# ---------------------------------------------------------------------------------------------
# dropout on the probabilities
# ---------------------------------------------------------------------------------------------
DROP_SHAPES = [(65, 3, 32), (129, 1, 64)]
DROP_IDS = [f"L{l}_H{h}_dh{dh}" for l, h, dh in DROP_SHAPES]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("l,h,dh", DROP_SHAPES, ids=DROP_IDS)
def test_pad_dropout(l, h, dh, p, dev):
    from vidsitu_amd import ops

    d = h * dh
    for kind in ro.MASKS:
        c, qkv_d, dout_d, mask_d = _pad_case(ops, dev, R, l, h, dh, kind)
        cd = rd._attn_drop_case(R, l, h, dh, kind, p)
        drop = rd._drop(dev, rd.SEED, rd.ATTN_STEP, rd.ATTN_SITE, p)
        name = f"attn_tiled pad drop R{R} L{l} H{h} dh{dh} {kind} p={p}"
        out = _fwd(ops, qkv_d, mask_d, R, l, h, dh, False, drop)
        ro._check(name + " fwd", out, cd["o64"], cd["o32"])
        rd._zeros_stay_zero(name + " fwd", out, cd["o64"])
        assert torch.equal(out, _fwd(ops, qkv_d, mask_d, R, l, h, dh, False, drop)), name + ": forward runs differ"
        dqkv = _bwd(ops, qkv_d, mask_d, dout_d, R, l, h, dh, False, drop)
        _parts(name, ro._check, dqkv, cd["g64"], cd["g32"], d)
        for i in range(3):
            rd._zeros_stay_zero(name, dqkv[:, i * d:(i + 1) * d], cd["g64"][:, i * d:(i + 1) * d])
        assert torch.equal(dqkv, _bwd(ops, qkv_d, mask_d, dout_d, R, l, h, dh, False, drop)), name + ": backward runs differ"


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("l,h,dh", DROP_SHAPES, ids=DROP_IDS)
def test_causal_dropout(l, h, dh, p, dev):
    from vidsitu_amd import ops

    d = h * dh
    for kind in CAUSAL_MASKS:
        c = gd._attn_case(R, l, h, dh, kind, p)
        drop = gd._drop(dev, gd.SEED, gd.ATTN_STEP, gd.ATTN_SITE, p)
        name = f"attn_tiled causal drop R{R} L{l} H{h} dh{dh} {kind} p={p}"
        qkv_d, dout_d = c["qkv"].to(dev), c["dout"].to(dev)
        mask_d = None if c["mask"] is None else c["mask"].to(dev)
        out = _fwd(ops, qkv_d, mask_d, R, l, h, dh, True, drop)
        assert bool(torch.isfinite(out).all())
        ok = ~c["fm"]
        go._check(name + " fwd", out[ok.to(dev)], c["out64"][ok], c["out32"][ok])
        assert torch.equal(out, _fwd(ops, qkv_d, mask_d, R, l, h, dh, True, drop)), name + ": forward runs differ"
        dqkv = _bwd(ops, qkv_d, mask_d, dout_d, R, l, h, dh, True, drop)
        _parts(name, go._check, dqkv, c["g64"], c["g32"], d)
        assert torch.equal(dqkv, _bwd(ops, qkv_d, mask_d, dout_d, R, l, h, dh, True, drop)), name + ": backward runs differ"


@pytest.mark.parametrize("causal", [False, True], ids=["pad", "causal"])
def test_resident_forward_meets_tiled_backward(causal, dev):
    """One shape both families hold, p = 0.1: the resident forward and the tiled backward see the same mask -- it is a
    function of the element, not of the family -- so the tiled gradient meets the bound against the fp64 reference the
    resident pair is held to, and the resident pair does too."""
    from vidsitu_amd import ops

    l, h, dh, p, kind = 65, 3, 32, 0.1, "right"
    d = h * dh
    lib = ops._lib.load()
    assert lib.vs_attn_resident_fits(int(causal), l, dh, 0) == 1 and lib.vs_attn_resident_fits(int(causal), l, dh, 1) == 1
    if causal:
        c = gd._attn_case(R, l, h, dh, kind, p)
        drop = gd._drop(dev, gd.SEED, gd.ATTN_STEP, gd.ATTN_SITE, p)
        mask_d = c["mask"].to(dev)
        o64, o32, g64, g32, check = c["out64"], c["out32"], c["g64"], c["g32"], go._check
        res_fwd, res_bwd = ops.attn_causal, ops.attn_causal_bwd
    else:
        c = ro._attn_case(R, l, h, dh, kind)
        cd = rd._attn_drop_case(R, l, h, dh, kind, p)
        drop = rd._drop(dev, rd.SEED, rd.ATTN_STEP, rd.ATTN_SITE, p)
        mask_d = c["mask"].to(torch.uint8).to(dev)
        o64, o32, g64, g32, check = cd["o64"], cd["o32"], cd["g64"], cd["g32"], ro._check
        res_fwd, res_bwd = ops.attn_pad, ops.attn_pad_bwd
    qkv_d, dout_d = c["qkv"].to(dev), c["dout"].to(dev)
    name = f"attn {'causal' if causal else 'pad'} R{R} L{l} H{h} dh{dh} {kind} p={p}"
    check(name + " resident fwd", res_fwd(qkv_d, mask_d, R, l, h, drop=drop), o64, o32)
    check(name + " tiled fwd", _fwd(ops, qkv_d, mask_d, R, l, h, dh, causal, drop), o64, o32)
    _parts(name + " resident bwd", check, res_bwd(qkv_d, mask_d, dout_d, R, l, h, drop=drop), g64, g32, d)
    _parts(name + " tiled bwd", check, _bwd(ops, qkv_d, mask_d, dout_d, R, l, h, dh, causal, drop), g64, g32, d)


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [0, 1])
def test_refusals_write_nothing(causal, dev):
    """dh = 48, a scratch one byte short, a dropout threshold without the step's snapshot: an error, outputs untouched."""
    from vidsitu_amd import ops

    def attempt(r, l, h, dh, ws_bytes, snap, thr):
        d = h * dh
        qkv = torch.randn(r * l, 3 * d, device=dev)
        dout = torch.randn(r * l, d, device=dev)
        out = torch.full((r * l, d), 7.0, device=dev)
        dqkv = torch.full((r * l, 3 * d), 7.0, device=dev)
        ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=dev)
        if ws_bytes is None:  # the forward is under test as well
            with pytest.raises(ops._lib.VsError):
                ops._lib.call("vs_attn_tiled_fwd", ops._ptr(qkv), None, ops._ptr(out), r, l, h, dh, causal,
                              ops._ptr(snap), 1, thr, 1.0, ops._stream())
        with pytest.raises(ops._lib.VsError):
            ops._lib.call("vs_attn_tiled_bwd", ops._ptr(qkv), None, ops._ptr(dout), ops._ptr(dqkv), ops._ptr(ws),
                          (1 << 20) if ws_bytes is None else ws_bytes, r, l, h, dh, causal, ops._ptr(snap), 1, thr, 1.0,
                          ops._stream())
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((dqkv == 7.0).all()) and bool((ws == 7).all())

    attempt(2, 8, 1, 48, None, None, 0)
    attempt(2, 70, 2, 32, 2 * 2 * 3 * 70 * 4 - 1, None, 0)
    attempt(2, 70, 2, 32, None, None, ops.dropout_params(0.1)[0])
