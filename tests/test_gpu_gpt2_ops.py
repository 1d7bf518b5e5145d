"""Per-kernel parity of the GPT-2 decoder kernels (csrc/gpt2_ops.hip) with plain fp64 torch restatements,
at the shapes where their branches turn: the unrolled / tail loops of colsum, more than 64 keys or head
channels and left padding in the causal attention (forward and backward), every instantiation of the
ancestry decode kernel and the generic fallback past t = 64, the grid-stride loop of the elementwise
kernels, ld > V / no counted row / tiny vocabularies in the cross entropy, pos0 > 0 and out-of-range
tokens in the embedding.

Tolerance (docs/gpt2_ops_parity.md holds the measured table): every case evaluates the same restatement in
fp32 torch on the CPU; its error against fp64, max |diff| / max |fp64|, is the restatement's own fp32 noise
floor `e32`.  The kernel's error, measured the same way, must be at most 16 * e32 (another summation order,
the device's expf / tanhf) and never above the project's ceiling for fp32 kernels, 2e-4.  Exact-copy kernels
are compared bit for bit.  Every figure is printed (`PARITY ...`) before it is asserted.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FACTOR = 16.0
CEILING = 2e-4
NAN = float("nan")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _errs(got, ref64, ref32):
    ref64 = ref64.detach()
    scale = float(ref64.abs().max()) or 1.0
    e32 = float((ref32.detach().double() - ref64).abs().max()) / scale
    err = float((got.detach().cpu().double() - ref64).abs().max()) / scale
    return e32, err


def _check(name, got, ref64, ref32):
    """kernel error <= min(16 * e32, 2e-4), both relative to max |fp64 reference|."""
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    e32, err = _errs(got, ref64, ref32)
    print(f"PARITY {name} e32={e32:.3e} err={err:.3e}")
    assert err <= min(FACTOR * e32, CEILING), f"{name}: kernel error {err:.3e} vs fp32 floor {e32:.3e}"


# ---------------------------------------------------------------------------------------------
# colsum_f32
# ---------------------------------------------------------------------------------------------
COLSUM_CASES = [(1, 64), (16, 1), (17, 100), (112, 64), (113, 130), (129, 64), (240, 192), (241, 97),
                (600, 1024), (1000, 50)]


@pytest.mark.parametrize("m,n", COLSUM_CASES, ids=[f"{m}x{n}" for m, n in COLSUM_CASES])
def test_colsum_f32(m, n, dev):
    """Both loops (the unrolled one needs m + 112 < M: 112 / 113 are the last M without and the first with wave 0 in
    it, at 129 every wave is in it and wave 0 has a tail row; 240 / 241 the same edge one trip later), N % 64 != 0
    (clamped lanes) and N < 64."""
    from vidsitu_amd import ops

    x = torch.randn(m, n, generator=_gen(1000 * m + n))
    ref64, ref32 = x.double().sum(0), x.sum(0)
    xd = x.to(dev)
    a = ops.colsum_f32(xd)
    _check(f"colsum_f32 {m}x{n}", a, ref64, ref32)
    # out=: a view into a larger buffer -- nothing past column N is written, the bits repeat
    buf = torch.full((n + 64,), NAN, device=dev)
    b = ops.colsum_f32(xd, out=buf[:n])
    torch.cuda.synchronize()
    assert torch.equal(a, b), "two runs differ (the kernel claims a fixed summation order)"
    assert bool(torch.isnan(buf[n:]).all()), "colsum wrote past column N"


# ---------------------------------------------------------------------------------------------
# causal attention, forward and backward
# ---------------------------------------------------------------------------------------------
def _key_mask(kind, r, l):
    if kind == "none":
        return None
    m = torch.ones(r, l, dtype=torch.uint8)
    for row in range(r):
        if kind == "right":
            npad = (l // 4 + 1, 0, 2)[row % 3]
            m[row, l - npad:] = 0
        else:  # left padding: pads in front
            npad = {"left": (0, 5, 17), "left_small": (1, 3)}[kind][row]
            m[row, :npad] = 0
    return m


def _attn_ref(qkv, mask, r, l, h, dh, fm=None):
    """modeling_gpt2 Attention._attn in qkv's dtype.  fm [R, L] bool: queries whose every visible key is masked
    get their scores as fp32(dot) + (-1e4f) formed in fp32 (what the kernel and the model it mirrors do; one ulp
    there is 2^-10), then everything continues in the working dtype."""
    dt = qkv.dtype
    x = qkv.view(r, l, 3, h, dh)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))  # [R, H, L, dh]
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    causal = torch.ones(l, l, dtype=torch.bool).tril()
    s = torch.where(causal, s, torch.full((), -1e4, dtype=dt))  # a constant: no gradient by construction
    if mask is not None:
        add = (1.0 - mask.to(dt))[:, None, None, :] * -1e4
        if fm is not None and bool(fm.any()):
            s = torch.where(fm[:, None, :, None], (s.float() + add.float()).to(dt), s + add)
        else:
            s = s + add
    p = torch.softmax(s, -1)
    return (p @ v).transpose(1, 2).reshape(r * l, h * dh)


@functools.lru_cache(maxsize=None)
def _attn_case(r, l, h, dh, kind, loss_on_masked=False):
    """Inputs and the fp64 / fp32 references of one case, computed once for the forward and backward tests."""
    g = _gen(7 + 1000 * l + dh)
    d = h * dh
    qkv = torch.randn(r * l, 3 * d, generator=g)
    dout = torch.randn(r * l, d, generator=g)
    mask = _key_mask(kind, r, l)
    fm = torch.zeros(r, l, dtype=torch.bool) if mask is None else mask.long().cumsum(1) == 0
    if not loss_on_masked:
        # fully masked queries carry no loss in training: dout = 0 there (their probabilities are only good to
        # exp(+-2^-10), see test_attn_causal_fwd; the rows around them keep the normal bound)
        dout[fm.reshape(-1)] = 0.0
    q64 = qkv.double().requires_grad_(True)
    out64 = _attn_ref(q64, mask, r, l, h, dh, fm)
    g64, = torch.autograd.grad(out64, q64, dout.double())
    q32 = qkv.clone().requires_grad_(True)
    out32 = _attn_ref(q32, mask, r, l, h, dh)
    g32, = torch.autograd.grad(out32, q32, dout)
    return dict(qkv=qkv, dout=dout, mask=mask, fm=fm.reshape(-1), out64=out64.detach(), out32=out32.detach(),
                g64=g64, g32=g32)


ATTN_CASES = [(2, 1, 2, 16, "none"), (2, 16, 2, 16, "none"), (2, 17, 3, 32, "right"), (2, 60, 2, 64, "right"),
              (1, 65, 2, 64, "none"), (1, 130, 1, 16, "right"), (2, 20, 2, 128, "none"), (1, 33, 2, 80, "none"),
              (3, 24, 2, 64, "left")]
ATTN_IDS = [f"R{r}_L{l}_H{h}_dh{dh}_{k}" for r, l, h, dh, k in ATTN_CASES]
FULLY_MASKED_BOUND = 4e-3  # of max |v|: two roundings at 2^-10 on both sides of a convex combination of V rows


@pytest.mark.parametrize("r,l,h,dh,kind", ATTN_CASES, ids=ATTN_IDS)
def test_attn_causal_fwd(r, l, h, dh, kind, dev):
    from vidsitu_amd import ops

    c = _attn_case(r, l, h, dh, kind)
    name = f"attn_causal_fwd R{r} L{l} H{h} dh{dh} {kind}"
    mask_d = None if c["mask"] is None else c["mask"].to(dev)
    out = ops.attn_causal(c["qkv"].to(dev), mask_d, r, l, h)
    assert bool(torch.isfinite(out).all())
    ok = ~c["fm"]
    _check(name, out[ok.to(dev)], c["out64"][ok], c["out32"][ok])
    if bool(c["fm"].any()):
        # fully masked queries: future keys take softmax weight; held to the fp32-formed scores of the model
        fm = c["fm"]
        vmax = float(c["qkv"][:, 2 * h * dh:].abs().max())
        err = float((out[fm.to(dev)].cpu().double() - c["out64"][fm]).abs().max()) / vmax
        print(f"PARITY {name} [fully masked queries, of max|v|] bound={FULLY_MASKED_BOUND:.1e} err={err:.3e}")
        assert err <= FULLY_MASKED_BOUND
    assert torch.equal(out, ops.attn_causal(c["qkv"].to(dev), mask_d, r, l, h))


def _attn_bwd_poisoned(ops, qkv_d, mask_d, dout_d, r, l, h, dh, dev):
    """vs_attn_causal_bwd through the C ABI with dqkv and the whole scratch workspace full of NaN."""
    need = ops._lib.load().vs_attn_causal_bwd_scratch_bytes(r, l, h)
    ws = ops._workspace(need, dev)
    ws.view(torch.float32).fill_(NAN)
    dqkv = torch.full_like(qkv_d, NAN)
    ops._lib.call("vs_attn_causal_bwd", ops._ptr(qkv_d), ops._ptr(mask_d), ops._ptr(dout_d), ops._ptr(dqkv),
                  ops._ptr(ws), ws.numel(), r, l, h, dh, ops._stream())
    return dqkv


@pytest.mark.parametrize("r,l,h,dh,kind", ATTN_CASES, ids=ATTN_IDS)
def test_attn_causal_bwd(r, l, h, dh, kind, dev):
    """dqkv and the scratch start as NaN: every output has an owner and no stale scratch is read.  dq, dk and dv are
    compared as the three thirds of dqkv.  In the left-padding case the fully masked queries have dout = 0 (no loss
    at padding positions); the rows after them hold the normal bound with the mask present."""
    from vidsitu_amd import ops

    c = _attn_case(r, l, h, dh, kind)
    d = h * dh
    qkv_d, dout_d = c["qkv"].to(dev), c["dout"].to(dev)
    mask_d = None if c["mask"] is None else c["mask"].to(dev)
    dqkv = _attn_bwd_poisoned(ops, qkv_d, mask_d, dout_d, r, l, h, dh, dev)
    assert bool(torch.isfinite(dqkv).all()), "an element of dqkv has no owner, or NaN scratch / LDS was read"
    for i, part in enumerate(("dq", "dk", "dv")):
        sl = slice(i * d, (i + 1) * d)
        _check(f"attn_causal_bwd R{r} L{l} H{h} dh{dh} {kind} {part}", dqkv[:, sl], c["g64"][:, sl], c["g32"][:, sl])
    again = ops.attn_causal_bwd(qkv_d, mask_d, dout_d, r, l, h)
    assert torch.equal(dqkv, again), "two runs differ (the kernel claims a fixed summation order)"


def test_attn_causal_bwd_loss_on_fully_masked_queries(dev):
    """A fully masked query that does carry a gradient is the only place where dS_ij != 0 for a future key j > i:
    dV_j must take it (sum over every i), dK_j and dQ_i must not (the future score is a constant).  Row 0 has one
    pad in front, row 1 three, so at most nm = 3 such queries add into one output element.  Their probabilities
    are good to about 4e-3 relative (test_attn_causal_fwd), and each contribution is no larger than the slice's
    largest element, hence the bound nm * 4e-3 of the slice's max; taking the future keys into dK or leaving them
    out of dV moves elements by a whole contribution, two orders above it."""
    from vidsitu_amd import ops

    r, l, h, dh, nm = 2, 20, 2, 16, 3
    c = _attn_case(r, l, h, dh, "left_small", True)
    assert int(c["fm"].sum()) == 4 and float(c["dout"][c["fm"]].abs().min()) > 0
    d = h * dh
    qkv_d, dout_d, mask_d = c["qkv"].to(dev), c["dout"].to(dev), c["mask"].to(dev)
    dqkv = _attn_bwd_poisoned(ops, qkv_d, mask_d, dout_d, r, l, h, dh, dev)
    assert bool(torch.isfinite(dqkv).all())
    for i, part in enumerate(("dq", "dk", "dv")):
        sl = slice(i * d, (i + 1) * d)
        ref = c["g64"][:, sl]
        err = float((dqkv[:, sl].cpu().double() - ref).abs().max()) / float(ref.abs().max())
        print(f"PARITY attn_causal_bwd R{r} L{l} H{h} dh{dh} left_small+loss {part} "
              f"bound={nm * FULLY_MASKED_BOUND:.1e} err={err:.3e}")
        assert err <= nm * FULLY_MASKED_BOUND, part


# ---------------------------------------------------------------------------------------------
# decode attention
# ---------------------------------------------------------------------------------------------
def _decode_ref(qkv, kc, vc, anc, kmask, t, h, dh):
    dt = qkv.dtype
    rows = qkv.shape[0]
    x = qkv.view(rows, 3, h, dh)
    q, k_new, v_new = x[:, 0], x[:, 1], x[:, 2]  # [rows, H, dh]
    src = anc[:, :t].long() if anc is not None else torch.arange(rows)[:, None].expand(rows, t)
    pos = torch.arange(t)[None].expand(rows, t)
    k = torch.cat([kc.to(dt).permute(0, 2, 1, 3)[src, pos], k_new[:, None]], 1)  # [rows, t + 1, H, dh]
    v = torch.cat([vc.to(dt).permute(0, 2, 1, 3)[src, pos], v_new[:, None]], 1)
    s = torch.einsum("rhd,rjhd->rhj", q, k) / math.sqrt(dh)
    if kmask is not None:
        s = s + (1.0 - kmask[:, None, :t + 1].to(dt)) * -1e4
    return torch.einsum("rhj,rjhd->rhd", torch.softmax(s, -1), v).reshape(rows, h * dh)


def _decode_inputs(g, rows, h, dh, lmax, t, use_anc, use_mask):
    qkv = torch.randn(rows, 3 * h * dh, generator=g)
    kc = torch.randn(rows, h, lmax, dh, generator=g)
    vc = torch.randn(rows, h, lmax, dh, generator=g)
    kc[:, :, t:] = NAN  # a read at or past t that is not this step's own row shows
    vc[:, :, t:] = NAN
    anc = torch.randint(0, rows, (rows, lmax), generator=g).to(torch.int32) if use_anc else None
    kmask = None
    if use_mask:  # a few zeros among positions <= t, never all of them
        kmask = torch.ones(rows, lmax, dtype=torch.uint8)
        for r in range(rows):
            nz = min(3, t)
            kmask[r, torch.randperm(t + 1, generator=g)[:nz]] = 0
        kmask[:, t + 1:] = torch.randint(0, 2, (rows, lmax - t - 1), generator=g).to(torch.uint8)
    return qkv, kc, vc, anc, kmask


def _decode_check(ops, dev, name, qkv, kc, vc, anc, kmask, t, h, dh, packed, qkv_d=None):
    rows, d = qkv.shape[0], h * dh
    qkv_d = qkv.to(dev) if qkv_d is None else qkv_d
    kc_d, vc_d = kc.to(dev), vc.to(dev)
    out = ops.attn_decode(qkv_d, kc_d, vc_d, None if kmask is None else kmask.to(dev), t,
                          ancestry=None if anc is None else anc.to(dev), out_packed=packed)
    if packed:
        out = ops.unpack_rows_f32(out, rows, d)
    _check(name, out, _decode_ref(qkv.double(), kc, vc, anc, kmask, t, h, dh),
           _decode_ref(qkv, kc, vc, anc, kmask, t, h, dh))
    # the cache rows at t hold this step's k / v exactly, nothing else changed (NaN included: compare bits)
    x = qkv.view(rows, 3, h, dh)
    for which, cache, cache_d, new in (("k", kc, kc_d, x[:, 1]), ("v", vc, vc_d, x[:, 2])):
        want = cache.clone()
        want[:, :, t] = new
        assert torch.equal(_bits(cache_d.cpu()), _bits(want)), f"{name}: {which} cache"


DECODE_CASES = [  # rows, H, dh, Lmax, t list, ancestry, kmask, packed
    (5, 2, 16, 72, (0, 1, 63, 64, 70), True, False, False),
    (20, 2, 32, 40, (0, 15, 16, 17, 33), True, True, True),
    (40, 2, 64, 64, (31, 59, 63), True, False, True),
    (3, 1, 128, 70, (5, 65), True, True, False),
    (4, 3, 64, 24, (7,), False, True, False),
    (4, 2, 24, 70, (0, 9, 66), False, True, False),  # dh outside {16, 32, 64, 128}: the generic kernel
]


@pytest.mark.parametrize("rows,h,dh,lmax,ts,use_anc,use_mask,packed", DECODE_CASES,
                         ids=[f"rows{c[0]}_H{c[1]}_dh{c[2]}_Lmax{c[3]}" for c in DECODE_CASES])
def test_attn_decode(rows, h, dh, lmax, ts, use_anc, use_mask, packed, dev):
    from vidsitu_amd import ops

    g = _gen(100 * rows + dh)
    for t in ts:
        a = _decode_inputs(g, rows, h, dh, lmax, t, use_anc, use_mask)
        name = (f"attn_decode rows{rows} H{h} dh{dh} Lmax{lmax} t{t}"
                f"{' anc' if use_anc else ''}{' kmask' if use_mask else ''}{' packed' if packed else ''}")
        _decode_check(ops, dev, name, *a, t, h, dh, packed)


def test_attn_decode_misaligned_qkv_takes_generic_kernel(dev):
    """qkv offset by one float fails the 16-byte test, so dh = 64 runs the generic kernel; that kernel has neither
    ancestry tables nor packed outputs, and asking for them is a bad-argument error that launches nothing."""
    from vidsitu_amd import ops

    rows, h, dh, lmax, t = 4, 2, 64, 24, 9
    g = _gen(64)
    qkv, kc, vc, _, _ = _decode_inputs(g, rows, h, dh, lmax, t, False, False)
    flat = torch.zeros(qkv.numel() + 4, device=dev)
    flat[1:1 + qkv.numel()] = qkv.reshape(-1).to(dev)
    qkv_d = flat[1:1 + qkv.numel()].view(rows, 3 * h * dh)
    assert qkv_d.data_ptr() % 16 == 4
    _decode_check(ops, dev, f"attn_decode rows{rows} H{h} dh{dh} Lmax{lmax} t{t} misaligned", qkv, kc, vc, None,
                  None, t, h, dh, False, qkv_d=qkv_d)

    def refused(qkv_x, kc_x, vc_x, **kw):
        kc_d, vc_d = kc_x.to(dev), vc_x.to(dev)
        with pytest.raises(ops._lib.VsError, match="vs_status"):
            ops.attn_decode(qkv_x, kc_d, vc_d, None, t, **kw)
        torch.cuda.synchronize()
        assert torch.equal(_bits(kc_d.cpu()), _bits(kc_x)) and torch.equal(_bits(vc_d.cpu()), _bits(vc_x))

    anc = torch.randint(0, rows, (rows, lmax), generator=g).to(torch.int32).to(dev)
    refused(qkv_d, kc, vc, ancestry=anc)
    refused(qkv_d, kc, vc, out_packed=True)
    qkv24, kc24, vc24, _, _ = _decode_inputs(g, rows, h, 24, lmax, t, False, False)
    refused(qkv24.to(dev), kc24, vc24, ancestry=anc)
    refused(qkv24.to(dev), kc24, vc24, out_packed=True)


# ---------------------------------------------------------------------------------------------
# elementwise kernels
# ---------------------------------------------------------------------------------------------
EW_N = [1, 255, 256, 257, 1048576, 1048577, 2457600]  # the grid is capped at 4096 x 256 = 1 048 576 threads
GELU_K, GELU_C = math.sqrt(2.0 / math.pi), 0.044715


def _gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(GELU_K * (x + GELU_C * x * x * x)))


def _gelu_new_grad(x):
    t = torch.tanh(GELU_K * (x + GELU_C * x * x * x))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * GELU_K * (1.0 + 3.0 * GELU_C * x * x)


@functools.lru_cache(maxsize=None)
def _ew_inputs(n):
    g = _gen(n)
    x = torch.rand(n, generator=g) * 12.0 - 6.0
    dy = torch.randn(n, generator=g)
    if n >= 4:  # exact 0 and saturation on both sides, unit upstream gradient there
        x[:3] = torch.tensor([0.0, 20.0, -20.0])
        dy[:3] = 1.0
        x[-1] = 20.0
        dy[-1] = 1.0
    return x, dy


@pytest.mark.parametrize("n", EW_N)
def test_gelu_new_fwd(n, dev):
    from vidsitu_amd import ops

    x, _ = _ew_inputs(n)
    xd = x.to(dev)
    y = ops.gelu_new_fwd(xd)
    _check(f"gelu_new_fwd n={n}", y, _gelu_new(x.double()), _gelu_new(x))
    out = torch.full_like(xd, NAN)
    ops._lib.call("vs_gelu_new_fwd", ops._ptr(xd), ops._ptr(out), n, ops._stream())
    assert torch.equal(out, y), "an element of a NaN-filled output was not written"
    if n >= 4:
        assert y[:3].tolist() == [0.0, 20.0, 0.0] and float(y[-1]) == 20.0


@pytest.mark.parametrize("n", EW_N)
def test_gelu_new_bwd(n, dev):
    from vidsitu_amd import ops

    x, dy = _ew_inputs(n)
    xd, dyd = x.to(dev), dy.to(dev)
    dx = ops.gelu_new_bwd(dyd, xd)
    _check(f"gelu_new_bwd n={n}", dx, dy.double() * _gelu_new_grad(x.double()), dy * _gelu_new_grad(x))
    out = torch.full_like(xd, NAN)
    ops._lib.call("vs_gelu_new_bwd", ops._ptr(dyd), ops._ptr(xd), ops._ptr(out), n, ops._stream())
    assert torch.equal(out, dx), "an element of a NaN-filled output was not written"
    if n >= 4:  # derivative 0.5 at 0, exactly 1 / 0 where tanh has saturated
        assert dx[:3].tolist() == [0.5, 1.0, 0.0] and float(dx[-1]) == 1.0


@pytest.mark.parametrize("n", EW_N)
def test_add_f32(n, dev):
    from vidsitu_amd import ops

    x, dy = _ew_inputs(n)
    out = torch.full((n,), NAN, device=dev)
    got = ops.add_f32(x.to(dev), dy.to(dev), out=out)
    assert torch.equal(got.cpu(), x + dy)
    assert torch.equal(ops.add_f32(x.to(dev), dy.to(dev)), got)


@pytest.mark.parametrize("n", EW_N)
def test_relu_bwd(n, dev):
    from vidsitu_amd import ops

    x, dy = _ew_inputs(n)
    y = torch.relu(x - 1.0)  # an exact zero wherever x <= 1
    if n >= 4:
        y[1] = 0.0
        y[2] = -0.0
    yd, dyd = y.to(dev), dy.to(dev)
    dx = ops.relu_bwd(dyd, yd)
    assert torch.equal(dx.cpu(), torch.where(y > 0, dy, torch.zeros_like(dy)))
    out = torch.full_like(yd, NAN)
    ops._lib.call("vs_relu_bwd", ops._ptr(dyd), ops._ptr(yd), ops._ptr(out), n, ops._stream())
    assert torch.equal(out, dx), "an element of a NaN-filled output was not written"


# ---------------------------------------------------------------------------------------------
# cross entropy with ignore_index
# ---------------------------------------------------------------------------------------------
IGNORE = 1
GRAD_SCALE = 0.37
N_LABEL_SETS = 8


def _xent_labels(g, rows, v, all_ignored=False):
    labels = torch.randint(0, v, (rows,), generator=g)
    labels[labels == IGNORE] = 0
    if rows > 1:
        labels[int(torch.randint(0, 3, (1,), generator=g))::3] = IGNORE  # some labels are ignored
        labels[0] = 0
    if all_ignored:
        labels[:] = IGNORE
    return labels


def _xent_inputs(rows, v, all_ignored=False):
    """logits, the labels the gradient is checked with, and N_LABEL_SETS label sets for the loss: one scalar's fp32
    floor can be almost 0 by luck (it was 4e-9 for 12 x 50259, below half an ulp of any fp32 result), so the loss
    is compared as a vector of losses over the same logits."""
    g = _gen(rows * 100003 + v)
    logits = torch.randn(rows, v, generator=g) * 3.0
    sets = [_xent_labels(g, rows, v, all_ignored) for _ in range(N_LABEL_SETS)]
    return logits, sets[0], sets


def _xent_ref(logits, labels, scale):
    x = logits.clone().requires_grad_(True)
    loss = F.cross_entropy(x, labels, ignore_index=IGNORE)
    g, = torch.autograd.grad(loss, x)
    return loss.detach(), g * scale


def _xent_losses(ops, dev, name, logits, label_sets, ld=None):
    """The mean losses of several label sets over the same logits, as one vector against F.cross_entropy."""
    rows, v = logits.shape
    wide = torch.full((rows, ld or v), NAN)  # NaN in the padding columns (ld > V) is never read
    wide[:, :v] = logits
    wide = wide.to(dev)
    got, l64, l32 = [], [], []
    for labels in label_sets:
        lb = labels.to(dev)
        if ld is None:
            loss, pair = ops.xent_ignore(wide, lb, IGNORE)
            assert float(loss) == float(pair[0])
        else:
            nll, pair = torch.full((rows,), NAN, device=dev), torch.full((2,), NAN, device=dev)
            ops._lib.call("vs_xent_ignore", ops._ptr(wide), ops._ptr(lb), ops._ptr(nll), ops._ptr(pair), rows, v, ld,
                          IGNORE, ops._stream())
        assert float(pair[1]) == int((labels != IGNORE).sum())
        got.append(pair[:1].cpu())
        l64.append(F.cross_entropy(logits.double(), labels, ignore_index=IGNORE).reshape(1))
        l32.append(F.cross_entropy(logits, labels, ignore_index=IGNORE).reshape(1))
    _check(f"xent_ignore {name} loss", torch.cat(got), torch.cat(l64), torch.cat(l32))
    return wide


def _xent_check(ops, dev, name, logits, labels, label_sets):
    """loss, count and the gradient through both grad_scale entry points (equal bits between the two)."""
    _xent_losses(ops, dev, name, logits, label_sets)
    _, g64 = _xent_ref(logits.double(), labels, GRAD_SCALE)
    _, g32 = _xent_ref(logits, labels, GRAD_SCALE)
    ld, lb = logits.to(dev), labels.to(dev)
    _, pair = ops.xent_ignore(ld, lb, IGNORE)
    dl = ops.xent_ignore_grad(ld, lb, pair, IGNORE, GRAD_SCALE)
    _check(f"xent_ignore_grad {name}", dl, g64, g32)
    dl_dev = ops.xent_ignore_grad(ld, lb, pair, IGNORE, torch.tensor([GRAD_SCALE], device=dev))
    assert torch.equal(dl, dl_dev), "host and device grad_scale give different bits"
    assert bool((dl[(labels == IGNORE).to(dev)] == 0).all())


XENT_CASES = [(1, 5), (7, 97), (40, 255), (40, 256), (40, 257), (12, 50259)]


@pytest.mark.parametrize("rows,v", XENT_CASES, ids=[f"{r}x{v}" for r, v in XENT_CASES])
def test_xent_ignore(rows, v, dev):
    from vidsitu_amd import ops

    logits, labels, label_sets = _xent_inputs(rows, v)
    _xent_check(ops, dev, f"{rows}x{v}", logits, labels, label_sets)


def test_xent_ignore_large_logits(dev):
    """+80 and -80 in one row: exp(80) overflows fp32 without the max subtraction; the label sits on the -80."""
    from vidsitu_amd import ops

    logits, labels, label_sets = _xent_inputs(7, 97)
    logits[0, 5], logits[0, 9], logits[2, 3] = 80.0, -80.0, 80.0
    for lb in label_sets:
        lb[0], lb[2] = 9, 3
    _xent_check(ops, dev, "7x97 +-80", logits, labels, label_sets)


def test_xent_ignore_every_label_ignored(dev):
    from vidsitu_amd import ops

    logits, labels, _ = _xent_inputs(7, 97, all_ignored=True)
    ld, lb = logits.to(dev), labels.to(dev)
    loss, pair = ops.xent_ignore(ld, lb, IGNORE)
    assert pair.tolist() == [0.0, 0.0] and float(loss) == 0.0
    for scale in (GRAD_SCALE, torch.tensor([GRAD_SCALE], device=dev)):
        dl = ops.xent_ignore_grad(ld, lb, pair, IGNORE, scale)
        assert bool(torch.isfinite(dl).all()) and bool((dl == 0).all())


def test_xent_ignore_row_pitch_above_vocab(dev):
    """ld = V + 3 through the C ABI: NaN in the padding columns of logits is never read, a sentinel in those of
    dlogits survives."""
    from vidsitu_amd import ops

    rows, v, pad, sentinel = 7, 97, 3, 12345.0
    logits, labels, label_sets = _xent_inputs(rows, v)
    wide = _xent_losses(ops, dev, f"{rows}x{v} ld={v + pad}", logits, label_sets, ld=v + pad)
    _, g64 = _xent_ref(logits.double(), labels, GRAD_SCALE)
    _, g32 = _xent_ref(logits, labels, GRAD_SCALE)
    lb = labels.to(dev)
    nll, pair = torch.full((rows,), NAN, device=dev), torch.full((2,), NAN, device=dev)
    ops._lib.call("vs_xent_ignore", ops._ptr(wide), ops._ptr(lb), ops._ptr(nll), ops._ptr(pair), rows, v, v + pad,
                  IGNORE, ops._stream())
    gs = torch.tensor([GRAD_SCALE], device=dev)
    outs = []
    for entry, scale in (("vs_xent_ignore_grad", GRAD_SCALE), ("vs_xent_ignore_grad_dev", ops._ptr(gs))):
        dl = torch.full((rows, v + pad), sentinel, device=dev)
        ops._lib.call(entry, ops._ptr(wide), ops._ptr(lb), ops._ptr(pair), ops._ptr(dl), rows, v, v + pad, IGNORE,
                      scale, ops._stream())
        assert bool((dl[:, v:] == sentinel).all()), f"{entry} wrote into the row padding"
        _check(f"{entry[3:]} {rows}x{v} ld={v + pad}", dl[:, :v], g64, g32)
        outs.append(dl)
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------
# embedding forward / backward, KV-cache gather
# ---------------------------------------------------------------------------------------------
def _embed_inputs(d, seed):
    g = _gen(seed)
    r, l, v, n_pos = 3, 5, 11, 16
    tok = torch.randint(0, v, (r, l), generator=g)
    tok[0, 1], tok[1, 1], tok[2, 4] = tok[0, 0], tok[0, 0], tok[0, 0]  # repeats, within and across rows
    tok[1, 3], tok[2, 0] = -1, v  # out of range on both sides
    bad = (tok < 0) | (tok >= v)
    wte = torch.randn(v, d, generator=g)
    wpe = torch.randn(n_pos, d, generator=g)
    return r, l, v, n_pos, tok, bad, wte, wpe, g


@pytest.mark.parametrize("pos0", [0, 7])
@pytest.mark.parametrize("d", [4, 64, 1024, 1028])
def test_gpt2_embed(d, pos0, dev):
    """Out-of-range tokens read row 0.  With one addend zero the kernel is an exact copy."""
    from vidsitu_amd import ops

    r, l, v, n_pos, tok, bad, wte, wpe, _ = _embed_inputs(d, 10 * d + pos0)
    safe = torch.where(bad, torch.zeros_like(tok), tok).reshape(-1)
    pos = (pos0 + torch.arange(l)).repeat(r)
    tok_d, wte_d, wpe_d = tok.to(dev), wte.to(dev), wpe.to(dev)
    out = ops.gpt2_embed(tok_d, wte_d, wpe_d, pos0)
    _check(f"gpt2_embed D={d} pos0={pos0}", out, wte.double()[safe] + wpe.double()[pos], wte[safe] + wpe[pos])
    assert torch.equal(ops.gpt2_embed(tok_d, wte_d, torch.zeros_like(wpe_d), pos0).cpu(), wte[safe])
    assert torch.equal(ops.gpt2_embed(tok_d, torch.zeros_like(wte_d), wpe_d, pos0).cpu(), wpe[pos])


@pytest.mark.parametrize("pos0", [0, 7])
@pytest.mark.parametrize("d", [4, 64, 1024, 1028])
def test_gpt2_embed_bwd(d, pos0, dev):
    """fp64 index_add_; atomics change only the order of the sum.  An out-of-range token adds nothing to dwte and
    (the kernel's behaviour, asserted as it is) nothing to dwpe either: its whole row is skipped."""
    from vidsitu_amd import ops

    r, l, v, n_pos, tok, bad, wte, wpe, g = _embed_inputs(d, 10 * d + pos0)
    dh = torch.randn(r * l, d, generator=g)
    keep = ~bad.reshape(-1)
    pos = (pos0 + torch.arange(l)).repeat(r)

    def ref(dt):
        dwte = torch.zeros(v, d, dtype=dt).index_add_(0, tok.reshape(-1)[keep], dh.to(dt)[keep])
        dwpe = torch.zeros(n_pos, d, dtype=dt).index_add_(0, pos[keep], dh.to(dt)[keep])
        return dwte, dwpe

    (dwte64, dwpe64), (dwte32, dwpe32) = ref(torch.float64), ref(torch.float32)
    dwte, dwpe = torch.zeros(v, d, device=dev), torch.zeros(n_pos, d, device=dev)
    ops.gpt2_embed_bwd(tok.to(dev), dh.to(dev), dwte, dwpe, pos0)
    _check(f"gpt2_embed_bwd D={d} pos0={pos0} dwte", dwte, dwte64, dwte32)
    _check(f"gpt2_embed_bwd D={d} pos0={pos0} dwpe", dwpe, dwpe64, dwpe32)
    untouched = torch.ones(n_pos, dtype=torch.bool)
    untouched[pos0:pos0 + l] = False
    assert bool((dwpe[untouched.to(dev)] == 0).all()) and bool((dwte[(dwte64 == 0).all(1).to(dev)] == 0).all())


@pytest.mark.parametrize("length", [0, 1, 6])
def test_kv_gather(length, dev):
    from vidsitu_amd import ops

    g = _gen(length)
    h, lmax, dh, sentinel = 2, 6, 8, -777.0
    src = torch.randn(4, h, lmax, dh, generator=g)
    index = torch.tensor([3, 0, 3, 1, 1, 2])
    dst = torch.full((6, h, lmax, dh), sentinel, device=dev)
    ops.kv_gather(src.to(dev), dst, index.to(dev), length)
    want = torch.full((6, h, lmax, dh), sentinel)
    want[:, :, :length] = src[index][:, :, :length]
    assert torch.equal(dst.cpu(), want)
