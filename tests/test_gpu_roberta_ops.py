"""The RoBERTa kernels (csrc/roberta_ops.hip) against fp64, case by case: padding-masked attention forward and
backward on the matrix instruction, the embedding rule, erf GELU and tanh.

Tolerance (the project's rule for fp32 kernels, as tests/test_gpu_gpt2_ops.py; docs/roberta_ops_parity.md holds the
measured table): every case evaluates the plain-torch restatement (tests/roberta_ref.py) in fp32 on the CPU; its error
against fp64, max |diff| / max |fp64|, is the restatement's own fp32 noise floor `e32`.  The kernel's error, measured
the same way, must be at most 16 * e32 and never above 2e-4.  A quantity whose fp64 value is exactly zero everywhere
(dq and dk of a one-token sequence) must be exactly zero.  Every figure is printed (`PARITY ...`) before it is asserted.
"""
import functools

import pytest
import torch

import roberta_ref as ref

pytestmark = pytest.mark.gpu

FACTOR = 16.0
CEILING = 2e-4
NAN = float("nan")
MASKS = ("none", "right", "left", "zero_row")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


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
    assert err <= min(FACTOR * e32, CEILING), f"{name}: kernel error {err:.3e} vs fp32 floor {e32:.3e}"


def _mask(kind, r, l):
    """{0,1} [R, L] or None.  right: differing lengths down to ONE valid key; left: padding at the start;
    zero_row: right padding with one sequence whose mask is all zero."""
    if kind == "none":
        return None
    m = torch.ones((r, l), dtype=torch.long)
    lens = [max(1, l - (i * (l // 2 + 1))) if i < r - 1 else 1 for i in range(r)]  # l, about l/2, ..., 1
    for i, n in enumerate(lens):
        if kind == "left":
            m[i, : l - n] = 0
        else:
            m[i, n:] = 0
    if kind == "zero_row":
        m[r - 1 if r > 1 else 0] = 0
    return m


@functools.lru_cache(maxsize=None)
def _attn_case(r, l, h, dh, kind):
    """Inputs and the fp64 / fp32 references (forward and gradients), computed once and left unchanged."""
    g = _gen(1000 * l + 10 * h + dh + len(kind))
    d = h * dh
    qkv = torch.randn(r, l, 3 * d, generator=g)
    qkv[..., : 2 * d] *= 1.5  # sharper softmax than unit-variance scores
    dout = torch.randn(r, l, d, generator=g)
    mask = _mask(kind, r, l)
    out = {}
    for dt in (torch.float64, torch.float32):
        x = qkv.to(dt).requires_grad_(True)
        o = ref.attention(x, mask, h)
        (gx,) = torch.autograd.grad(o, x, dout.to(dt))
        out[dt] = (o.detach().reshape(r * l, d), gx.reshape(r * l, 3 * d))
    return dict(qkv=qkv.reshape(r * l, 3 * d), dout=dout.reshape(r * l, d), mask=mask, o64=out[torch.float64][0],
                g64=out[torch.float64][1], o32=out[torch.float32][0], g32=out[torch.float32][1])


def _bwd_poisoned(ops, qkv_d, mask_d, dout_d, r, l, h, dh, dev):
    """vs_attn_pad_bwd through the C ABI with dqkv and the whole scratch workspace full of NaN."""
    need = ops._lib.load().vs_attn_pad_bwd_scratch_bytes(r, l, h)
    ws = ops._workspace(need, dev)
    ws.view(torch.float32).fill_(NAN)
    dqkv = torch.full_like(qkv_d, NAN)
    ops._lib.call("vs_attn_pad_bwd", ops._ptr(qkv_d), ops._ptr(mask_d), ops._ptr(dout_d), ops._ptr(dqkv),
                  ops._ptr(ws), ws.numel(), r, l, h, dh, ops._stream())
    return dqkv


@pytest.mark.parametrize("h", [1, 2, 12])
@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("l", [1, 5, 15, 16, 17, 60, 64, 65, 120])
def test_attn_pad_fwd_bwd(l, dh, h, dev):
    """Every mask kind at this shape: forward, then the backward into NaN-filled dqkv and scratch (every output has an
    owner, no stale scratch is read); dq, dk and dv are held to the bound separately; a second run of each agrees bit
    for bit."""
    from vidsitu_amd import ops

    r = 3
    d = h * dh
    for kind in MASKS:
        c = _attn_case(r, l, h, dh, kind)
        name = f"attn_pad R{r} L{l} H{h} dh{dh} {kind}"
        qkv_d, dout_d = c["qkv"].to(dev), c["dout"].to(dev)
        mask_d = None if c["mask"] is None else c["mask"].to(torch.uint8).to(dev)
        out = ops.attn_pad(qkv_d, mask_d, r, l, h)
        _check(name + " fwd", out, c["o64"], c["o32"])
        assert torch.equal(out, ops.attn_pad(qkv_d, mask_d, r, l, h)), name + ": forward runs differ"
        dqkv = _bwd_poisoned(ops, qkv_d, mask_d, dout_d, r, l, h, dh, dev)
        for i, part in enumerate(("dq", "dk", "dv")):
            sl = slice(i * d, (i + 1) * d)
            _check(f"{name} {part}", dqkv[:, sl], c["g64"][:, sl], c["g32"][:, sl])
        assert torch.equal(dqkv, ops.attn_pad_bwd(qkv_d, mask_d, dout_d, r, l, h)), name + ": backward runs differ"


def test_attn_pad_refuses_what_it_cannot_hold(dev):
    """A sequence longer than the LDS budget, or a head width outside {16, 32, 64, 128}: an error, nothing written."""
    from vidsitu_amd import ops

    for r, l, h, dh in ((1, 4096, 1, 64), (2, 8, 1, 48), (1, 200, 2, 128)):
        d = h * dh
        qkv = torch.randn(r * l, 3 * d, device=dev)
        dout = torch.randn(r * l, d, device=dev)
        out = torch.full((r * l, d), 7.0, device=dev)
        with pytest.raises(ops._lib.VsError):
            ops._lib.call("vs_attn_pad_fwd", ops._ptr(qkv), None, ops._ptr(out), r, l, h, dh, ops._stream())
        dqkv = torch.full((r * l, 3 * d), 7.0, device=dev)
        ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=dev)
        with pytest.raises(ops._lib.VsError):
            ops._lib.call("vs_attn_pad_bwd", ops._ptr(qkv), None, ops._ptr(dout), ops._ptr(dqkv), ops._ptr(ws),
                          1 << 62, r, l, h, dh, ops._stream())
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((dqkv == 7.0).all()) and bool((ws == 7).all())
    with pytest.raises(ops._lib.VsError):  # a scratch that is too small is refused too
        qkv = torch.randn(16, 3 * 32, device=dev)
        ws = torch.empty(16, dtype=torch.uint8, device=dev)
        ops._lib.call("vs_attn_pad_bwd", ops._ptr(qkv), None, ops._ptr(qkv), ops._ptr(torch.empty_like(qkv)),
                      ops._ptr(ws), ws.numel(), 1, 16, 1, 32, ops._stream())


# ---------------------------------------------------------------------------------------------
# embedding
# ---------------------------------------------------------------------------------------------
def _embed_tokens(r, l, vocab, pad, seed):
    g = _gen(seed)
    toks = torch.randint(4, vocab, (r, l), generator=g)
    toks[:, 0] = 0
    for i in range(1, r):
        n = max(2, l - 3 * i)
        toks[i, n:] = pad  # right padding
        toks[i, n - 1] = 2
    if l >= 6:
        toks[0, l // 2] = pad  # a pad token in the MIDDLE of a sequence: later tokens do not count it
    if r > 2:
        toks[2, 0] = pad  # and one at the start
    return toks


@pytest.mark.parametrize("r,l,d", [(1, 1, 4), (3, 7, 20), (4, 60, 64), (2, 120, 768), (2, 300, 36)])
def test_roberta_embed(r, l, d, dev):
    from vidsitu_amd import ops

    vocab, pad, n_pos = 53, 1, l + 2
    g = _gen(31 * l + d)
    word, pos, typ = (torch.randn(n, d, generator=g) for n in (vocab, n_pos, 1))
    toks = _embed_tokens(r, l, vocab, pad, 7 * l + r)
    w = {"embeddings.word_embeddings.weight": word, "embeddings.position_embeddings.weight": pos,
         "embeddings.token_type_embeddings.weight": typ}
    dims = {"pad_token_id": pad}
    e64, pid = ref.embed({k: v.double() for k, v in w.items()}, toks, dims)
    e32, _ = ref.embed(w, toks, dims)
    out, pos_ids = ops.roberta_embed(toks.to(dev), word.to(dev), pos.to(dev), typ.to(dev), pad)
    assert torch.equal(pos_ids.cpu(), pid), "position ids must be exactly those of the token ids"
    if l >= 6:
        assert int(pos_ids[0, l // 2]) == pad and int(pos_ids[0, l // 2 + 1]) == pad + l // 2 + 1
    _check(f"roberta_embed R{r} L{l} D{d}", out.view(r, l, d), e64, e32)
    # backward through the existing scatter kernel, once with the tokens and once with the position ids: the
    # padding rows of both tables stay zero (nn.Embedding(padding_idx = pad))
    de = torch.randn(r * l, d, generator=g)
    dword, dpos = torch.zeros(vocab, d, device=dev), torch.zeros(n_pos, d, device=dev)
    ops.embed_scatter_bwd(toks.to(dev), de.to(dev), dword, 1.0, pad)
    ops.embed_scatter_bwd(pos_ids, de.to(dev), dpos, 1.0, pad)
    assert float(dword[pad].abs().max()) == 0.0 and float(dpos[pad].abs().max()) == 0.0
    refs = {}
    for dt in (torch.float64, torch.float32):
        wl = {k: v.to(dt).requires_grad_(True) for k, v in w.items()}
        e, _ = ref.embed(wl, toks, dims)
        e.backward(de.to(dt).view(r, l, d))
        gw, gp = wl["embeddings.word_embeddings.weight"].grad.clone(), \
            wl["embeddings.position_embeddings.weight"].grad.clone()
        gw[pad], gp[pad] = 0, 0
        refs[dt] = (gw, gp, wl["embeddings.token_type_embeddings.weight"].grad)
    _check(f"roberta_embed R{r} L{l} D{d} dword", dword, refs[torch.float64][0], refs[torch.float32][0])
    _check(f"roberta_embed R{r} L{l} D{d} dpos", dpos, refs[torch.float64][1], refs[torch.float32][1])
    dtyp = ops.colsum_f32(de.to(dev))
    _check(f"roberta_embed R{r} L{l} D{d} dtype", dtyp.view(1, d), refs[torch.float64][2], refs[torch.float32][2])


def test_roberta_embed_refuses_a_short_position_table(dev):
    from vidsitu_amd import ops

    toks = torch.zeros((1, 8), dtype=torch.int64, device=dev)
    word, typ = torch.zeros(4, 8, device=dev), torch.zeros(1, 8, device=dev)
    ops.roberta_embed(toks, word, torch.zeros(10, 8, device=dev), typ, 1)  # 8 + 1 + 1 <= 10
    with pytest.raises(ops._lib.VsError):
        ops.roberta_embed(toks, word, torch.zeros(9, 8, device=dev), typ, 1)


# ---------------------------------------------------------------------------------------------
# activations: sizes that are no multiple of a vector, a wave or the block, and more than the grid's one pass
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [67, 257, 1000, 4096 * 256 + 5])  # (e32 of a handful of elements is no noise floor)
def test_gelu_erf_and_tanh(n, dev):
    from vidsitu_amd import ops

    g = _gen(n)
    x = torch.randn(n, generator=g) * 3.0
    dy = torch.randn(n, generator=g)
    r = {}
    for dt in (torch.float64, torch.float32):
        xx = x.to(dt).requires_grad_(True)
        y = ref.gelu(xx)
        (gx,) = torch.autograd.grad(y, xx, dy.to(dt))
        tt = x.to(dt).requires_grad_(True)
        t = torch.tanh(tt)
        (gt,) = torch.autograd.grad(t, tt, dy.to(dt))
        r[dt] = (y.detach(), gx, t.detach(), gt)
    xd, dyd = x.to(dev), dy.to(dev)
    _check(f"gelu_erf_fwd n{n}", ops.gelu_erf_fwd(xd), r[torch.float64][0], r[torch.float32][0])
    _check(f"gelu_erf_bwd n{n}", ops.gelu_erf_bwd(dyd, xd), r[torch.float64][1], r[torch.float32][1])
    y = ops.tanh_fwd(xd)
    _check(f"tanh_fwd n{n}", y, r[torch.float64][2], r[torch.float32][2])
    _check(f"tanh_bwd n{n}", ops.tanh_bwd(dyd, y), r[torch.float64][3], r[torch.float32][3])
