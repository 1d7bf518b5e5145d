"""The cross-attention kernels (csrc/attn_cross.hip) against fp64, case by case: forward, backward and the one-query
cached decode step with its cache split.

Tolerance (the project's rule for fp32 kernels, as tests/test_gpu_roberta_ops.py; docs/txdec_cross_parity.md holds the
measured table): every case evaluates the plain-torch restatement (tests/txdec_cross_ref.py) in fp32 on the CPU; its
error against fp64, max |diff| / max |fp64|, is the restatement's own fp32 noise floor `e32`.  The kernel's error,
measured the same way, must be at most 16 * e32 and never above 2e-4.  A quantity whose fp64 value is exactly zero
everywhere (dq and dk over a one-key source) must be exactly zero.  Every figure is printed (`PARITY ...`) before it is
asserted.
"""
import functools

import pytest
import torch

import txdec_cross_ref as ref

pytestmark = pytest.mark.gpu

FACTOR = 16.0
CEILING = 2e-4
NAN = float("nan")
MASKS = ("none", "right", "left", "zero_row")
R = 3


def _bound(e32):
    return min(FACTOR * e32, CEILING)


def _check(name, got, ref64, ref32):
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    ref64 = ref64.detach()
    got = got.detach().cpu().double()
    scale = float(ref64.abs().max())
    if scale == 0.0:
        print(f"PARITY {name} fp64 value is exactly zero, max |got| = {float(got.abs().max()):.3e}")
        assert float(got.abs().max()) == 0.0, f"{name}: must be exactly zero"
        return
    e32 = float((ref32.detach().double() - ref64).abs().max()) / scale
    err = float((got - ref64).abs().max()) / scale
    print(f"PARITY {name} e32={e32:.3e} err={err:.3e}")
    assert err <= _bound(e32), f"{name}: kernel error {err:.3e} vs fp32 floor {e32:.3e}"


def _mask(kind, r, s):
    """{0,1} [R, S] or None.  right: differing lengths down to ONE valid key; left: padding at the start;
    zero_row: right padding with one source whose mask is all zero."""
    if kind == "none":
        return None
    m = torch.ones((r, s), dtype=torch.long)
    lens = [max(1, s - (i * (s // 2 + 1))) if i < r - 1 else 1 for i in range(r)]  # s, about s/2, ..., 1
    for i, n in enumerate(lens):
        if kind == "left":
            m[i, : s - n] = 0
        else:
            m[i, n:] = 0
    if kind == "zero_row":
        m[r - 1 if r > 1 else 0] = 0
    return m


def _limit(dh, backward):
    """The longest source the kernels hold at this head width, read from vs_attn_cross_fits."""
    from vidsitu_amd import ops

    return max(s for s in range(1, 1025) if ops.attn_cross_fits(17, s, dh, backward))


@functools.lru_cache(maxsize=None)
def _case(l, s, h, dh, kind, grads=True):
    """Inputs and the fp64 / fp32 references (forward and gradients), computed once and left unchanged."""
    g = torch.Generator().manual_seed(100000 * l + 100 * s + 10 * h + dh + len(kind))
    d = h * dh
    q = torch.randn(R, l, d, generator=g) * 1.5  # sharper softmax than unit-variance scores
    kv = torch.randn(R, s, 2 * d, generator=g)
    kv[..., :d] *= 1.5
    dout = torch.randn(R, l, d, generator=g)
    mask = _mask(kind, R, s)
    out = {}
    for dt in (torch.float64, torch.float32):
        a, b = q.to(dt).requires_grad_(True), kv.to(dt).requires_grad_(True)
        o = ref.cross_attention(a, b, mask, h)
        ga, gb = torch.autograd.grad(o, (a, b), dout.to(dt)) if grads else (None, None)
        out[dt] = (o.detach().reshape(R * l, d), None if ga is None else ga.reshape(R * l, d),
                   None if gb is None else gb.reshape(R * s, 2 * d))
    return dict(q=q.reshape(R * l, d), kv=kv.reshape(R * s, 2 * d), dout=dout.reshape(R * l, d), mask=mask,
                r64=out[torch.float64], r32=out[torch.float32])


def _bwd_poisoned(ops, q, kv, mask, dout, l, s, h, dh, dev):
    """vs_attn_cross_bwd through the C ABI with dq, dkv and the whole scratch workspace full of NaN."""
    need = ops._lib.load().vs_attn_cross_bwd_scratch_bytes(R, l, s, h)
    ws = ops._workspace(need, dev)
    ws.view(torch.float32).fill_(NAN)
    dq, dkv = torch.full_like(q, NAN), torch.full_like(kv, NAN)
    ops._lib.call("vs_attn_cross_bwd", ops._ptr(q), ops._ptr(kv), ops._ptr(mask), ops._ptr(dout), ops._ptr(dq),
                  ops._ptr(dkv), ops._ptr(ws), ws.numel(), R, l, s, h, dh, ops._stream())
    return dq, dkv


SHAPES = [(1, 1), (1, 17), (5, 2), (16, 15), (17, 16), (60, 5), (65, 60), (17, "fwd_max"), (17, "bwd_max")]


@pytest.mark.parametrize("h", [1, 8])
@pytest.mark.parametrize("dh", [32, 128])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda t: f"L{t[0]}-S{t[1]}")
def test_attn_cross_fwd_bwd(shape, dh, h, dev):
    """Every mask kind at this shape: forward, then (where the backward holds S) the backward into NaN-filled dq, dkv
    and scratch (every output has an owner, no stale scratch is read); dq, dk and dv are held to the bound separately; a
    second run of each agrees bit for bit."""
    from vidsitu_amd import ops

    l, s = shape
    s = _limit(dh, False) if s == "fwd_max" else _limit(dh, True) if s == "bwd_max" else s
    back = ops.attn_cross_fits(l, s, dh, True)
    assert ops.attn_cross_fits(l, s, dh, False)
    assert back or shape[1] == "fwd_max", "only the forward's own limit lies past the backward's"
    d = h * dh
    for kind in MASKS:
        c = _case(l, s, h, dh, kind, back)
        name = f"attn_cross L{l} S{s} H{h} dh{dh} {kind}"
        q, kv, dout = c["q"].to(dev), c["kv"].to(dev), c["dout"].to(dev)
        mask = None if c["mask"] is None else c["mask"].to(torch.uint8).to(dev)
        out = ops.attn_cross(q, kv, mask, R, l, s, h)
        _check(name + " fwd", out, c["r64"][0], c["r32"][0])
        assert torch.equal(out, ops.attn_cross(q, kv, mask, R, l, s, h)), name + ": forward runs differ"
        if not back:
            continue
        dq, dkv = _bwd_poisoned(ops, q, kv, mask, dout, l, s, h, dh, dev)
        _check(name + " dq", dq, c["r64"][1], c["r32"][1])
        _check(name + " dk", dkv[:, :d], c["r64"][2][:, :d], c["r32"][2][:, :d])
        _check(name + " dv", dkv[:, d:], c["r64"][2][:, d:], c["r32"][2][:, d:])
        dq2, dkv2 = ops.attn_cross_bwd(q, kv, mask, dout, R, l, s, h)
        assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2), name + ": backward runs differ"


def test_attn_cross_refuses_what_it_cannot_hold(dev):
    """A source one key past each limit, a head width outside {16, 32, 64, 128} and a short scratch: an error that names
    the limit, nothing written."""
    from vidsitu_amd import ops

    lib = ops._lib
    for dh in (32, 128):
        fmax, bmax = _limit(dh, False), _limit(dh, True)
        assert bmax < fmax
        for l, s, h, w, fwd_ok in ((17, fmax + 1, 2, dh, False), (17, bmax + 1, 2, dh, True), (4, 8, 1, 48, False)):
            d = h * w
            q, kv = torch.randn(R * l, d, device=dev), torch.randn(R * s, 2 * d, device=dev)
            out = torch.full((R * l, d), 7.0, device=dev)
            if not fwd_ok:
                with pytest.raises(lib.VsError, match="limit|head width"):
                    lib.call("vs_attn_cross_fwd", ops._ptr(q), ops._ptr(kv), None, ops._ptr(out), R, l, s, h, w,
                             ops._stream())
            dq, dkv = torch.full_like(q, 7.0), torch.full_like(kv, 7.0)
            ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=dev)
            with pytest.raises(lib.VsError, match="limit|head width"):
                lib.call("vs_attn_cross_bwd", ops._ptr(q), ops._ptr(kv), None, ops._ptr(q), ops._ptr(dq),
                         ops._ptr(dkv), ops._ptr(ws), 1 << 62, R, l, s, h, w, ops._stream())
            torch.cuda.synchronize()
            assert bool((out == 7.0).all()) and bool((dq == 7.0).all()) and bool((dkv == 7.0).all())
            assert bool((ws == 7).all())
    # a scratch one byte short is refused too
    l, s, h, dh = 5, 7, 2, 32
    q, kv = torch.randn(R * l, h * dh, device=dev), torch.randn(R * s, 2 * h * dh, device=dev)
    need = lib.load().vs_attn_cross_bwd_scratch_bytes(R, l, s, h)
    assert need == R * h * 2 * l * 16 * 4
    dq, dkv = torch.full_like(q, 7.0), torch.full_like(kv, 7.0)
    ws = torch.full((need,), 7, dtype=torch.uint8, device=dev)
    with pytest.raises(lib.VsError, match="scratch"):
        lib.call("vs_attn_cross_bwd", ops._ptr(q), ops._ptr(kv), None, ops._ptr(q), ops._ptr(dq), ops._ptr(dkv),
                 ops._ptr(ws), need - 1, R, l, s, h, dh, ops._stream())
    torch.cuda.synchronize()
    assert bool((dq == 7.0).all()) and bool((dkv == 7.0).all()) and bool((ws == 7).all())


@pytest.mark.parametrize("h", [1, 8])
@pytest.mark.parametrize("dh", [32, 128])
@pytest.mark.parametrize("s", [1, 5, 60, "fwd_max"])
def test_attn_cross_decode_equals_the_forward_at_one_query(s, dh, h, dev):
    """The cached decode step (caches written by the split kernel) against fp64 and against the general forward kernel
    at L = 1, both within the bound; the split itself is a pure copy."""
    from vidsitu_amd import ops

    s = _limit(dh, False) if s == "fwd_max" else s
    d = h * dh
    for kind in MASKS:
        c = _case(1, s, h, dh, kind, False)
        name = f"attn_cross_decode S{s} H{h} dh{dh} {kind}"
        q, kv = c["q"].to(dev), c["kv"].to(dev)
        mask = None if c["mask"] is None else c["mask"].to(torch.uint8).to(dev)
        kc = torch.full((R, h, s, dh), NAN, device=dev)
        vc = torch.full((R, h, s, dh), NAN, device=dev)
        ops.attn_cross_kv_split(kv, kc, vc)
        kv4 = kv.view(R, s, 2, h, dh)
        assert torch.equal(kc, kv4[:, :, 0].transpose(1, 2)) and torch.equal(vc, kv4[:, :, 1].transpose(1, 2))
        out = ops.attn_cross_decode(q, kc, vc, mask)
        _check(name, out, c["r64"][0], c["r32"][0])
        assert torch.equal(out, ops.attn_cross_decode(q, kc, vc, mask)), name + ": runs differ"
        fwd = ops.attn_cross(q, kv, mask, R, 1, s, h)
        scale = float(c["r64"][0].abs().max())
        e32 = float((c["r32"][0].double() - c["r64"][0]).abs().max()) / scale
        diff = float((out - fwd).abs().max()) / scale
        print(f"PARITY {name} against the forward kernel e32={e32:.3e} diff={diff:.3e}")
        assert diff <= _bound(e32), f"{name}: decode and forward kernels differ by {diff:.3e}"
