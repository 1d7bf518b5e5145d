"""Every entry point of csrc/bn_pool.hip that the trunk runs, one pass at a time, against fp64 restatements of the same
bf16 / fp32 operands (tests/bn_pool_ref.py) at the shapes where the kernels' branches turn: generic and column-owner
BN kernels, C > 2048 (second trip of the column loop), rows around one block, nbatch 2 / 3 / 4 and its clamp, every
ReLU-mask arm, row pitches that all differ (outputs are channel slices of NaN-patterned buffers that must stay
untouched), the 64-bit index arms of the 3x3 pool, NaN / -inf / ties in every pool, the loop edges of the average
pool, the column sum and the row softmax.

Criteria (derived in bn_pool_ref.py, measured figures in docs/bn_pool_parity.md): bf16 results of fp32 arithmetic must
lie in [bf16(v64 - delta), bf16(v64 + delta)] with delta counted from the kernel's roundings and at most 1 % of a case's
elements ambiguous; ReLU decisions equal v64 > 0 outside delta (at most 0.1 % inside); selections and copies bit for
bit; fp32 sums within (chain + tree) * 2^-24 * sum |terms|; the softmax within 16 x the fp32 restatement's own error.
Every figure is printed (`PARITY ...`, pytest -s) before it is asserted."""
import pytest
import torch

import bn_pool_ref as R

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
BIG = 1 << 22  # elements from which operands are generated on the device


def _randn(shape, seed, dev, mul=1.0, add=0.0, dtype=BF16):
    n = 1
    for s in shape:
        n *= s
    if n >= BIG:
        x = torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    else:
        x = torch.randn(shape, generator=R.gen(seed)).to(dev)
    return (x * mul + add).to(dtype)


def _vec(c, seed, dev, kind):
    g = R.gen(seed)
    if kind == "pos":  # scale, gamma, invstd
        return (torch.rand(c, generator=g) + 0.5).to(dev)
    return (torch.randn(c, generator=g) * kind).to(dev)


def _slice(t, ld=None, off=0):
    """[rows, C] operand -> (buffer, view): with ld, a channel slice of a NaN-patterned [rows, ld] buffer."""
    if ld is None:
        t = t.contiguous()
        return t, t
    buf = R.nan_filled((t.shape[0], ld), t.device, t.dtype)
    buf[:, off:off + t.shape[1]] = t
    return buf, buf[:, off:off + t.shape[1]]


def _out(rows, c, dev, ld=None, off=0, dtype=BF16):
    buf = R.nan_filled((rows, ld or c), dev, dtype)
    return buf, buf[:, off:off + c]


def _api():
    from vidsitu_amd import ops

    return ops, ops._lib.call, ops._ptr, ops._stream


def _launches(ops):
    return int(ops._lib.load().vs_launch_count())


def _refused(ops, name, *args):
    """The entry point returns an error and launches nothing."""
    from vidsitu_amd._lib import VsError

    n0 = _launches(ops)
    with pytest.raises(VsError):
        ops._lib.call(name, *args)
    assert _launches(ops) == n0, f"{name} launched a kernel before refusing its arguments"


def _rl(c):
    return 256 // min(c // 8, 256)


def _pow2(c):
    return (c // 8) & (c // 8 - 1) == 0


def _edge_cases(cs):
    out = []
    for c in cs:
        e = _rl(c) * 4
        out += [(c, r, False) for r in (1, e - 1, e)] + [(c, e + 1, True)]
    return out


def _ids(cases):
    return [f"C{c}_rows{r}" + ("_pitched" if p else "") for c, r, p in cases]


# ---------------------------------------------------------------------------------------------
# BN apply: vs_bn_apply, vs_bn_apply_mask, vs_bn_apply2
# ---------------------------------------------------------------------------------------------
BN_APPLY_CASES = _edge_cases([8, 64, 2048, 4096]) + [(2048, r, False) for r in (8193, 16385, 24577, 40000)] \
    + [(c, r, r == 7) for c in (24, 72, 200) for r in (1, 7, 1000)] + [(72, 60000, False)]


@pytest.mark.parametrize("c,rows,pitched", BN_APPLY_CASES, ids=_ids(BN_APPLY_CASES))
def test_bn_apply(c, rows, pitched, dev):
    """Column-owner kernel (C/8 a power of two): rl = 256 / min(C/8, 256) row lanes x 4 rows per batch, so rows =
    1, 4 rl - 1, 4 rl, 4 rl + 1 are one row (every other lane re-reads row 0 and must not store), a block short of one
    row, one block, a second block of one row; C = 4096 takes a second trip of the column loop; C = 2048 with 8193 /
    16385 / 24577 / 40000 rows runs nbatch 2 / 3 / 4 / 4 (clamped).  Generic kernel (C = 24, 72, 200): per-element
    parameters, and at 60 000 x 72 more chunks than the 2048 x 256 threads of the capped grid (the stride loop wraps).
    Each with and without residual and ReLU; mask and RES_AFF arms where C/8 is a power of two; the pitched cases use
    three different row pitches and check every byte outside the output slice."""
    ops, call, P, S = _api()
    seed = 1000 * c + rows
    y = _randn((rows, c), seed, dev, 1.5, 0.3)
    res = _randn((rows, c), seed + 1, dev)
    scale, shift = _vec(c, seed + 2, dev, "pos"), _vec(c, seed + 3, dev, 0.3)
    ylo = (c + 8, 8) if pitched else (None, 0)
    rlo = (c + 24, 16) if pitched else (None, 0)
    olo = (c + 16, 8) if pitched else (None, 0)
    _, yv = _slice(y, *ylo)
    _, rv = _slice(res, *rlo)
    tag = f"C{c} rows{rows}" + (" pitched" if pitched else "")
    relu_out = {}
    for with_res in (False, True):
        r = rv if with_res else None
        v64, _, delta = R.bn_apply_ref(y, scale, shift, res if with_res else None)
        for relu in (0, 1):
            obuf, ov = _out(rows, c, dev, *olo)
            call("vs_bn_apply", P(yv), P(scale), P(shift), P(r), P(ov), rows, c, yv.stride(0), rv.stride(0) if with_res else 0,
                 ov.stride(0), relu, S())
            R.assert_interval(f"bn_apply {tag} res={int(with_res)} relu={relu}", ov, v64, delta, bool(relu))
            assert R.untouched(obuf, olo[1], c), "bn_apply wrote outside its channel slice"
            if relu:
                relu_out[with_res] = ov
        if not _pow2(c):
            bits = R.nan_filled((rows, c // 8), dev, torch.uint8)
            _, ov = _out(rows, c, dev, *olo)
            _refused(ops, "vs_bn_apply_mask", P(yv), P(scale), P(shift), P(r), P(ov), P(bits), rows, c, yv.stride(0),
                     rv.stride(0) if with_res else 0, ov.stride(0), S())
            continue
        bits = R.nan_filled((rows, c // 8), dev, torch.uint8)
        obuf, ov = _out(rows, c, dev, *olo)
        call("vs_bn_apply_mask", P(yv), P(scale), P(shift), P(r), P(ov), P(bits), rows, c, yv.stride(0),
             rv.stride(0) if with_res else 0, ov.stride(0), S())
        assert R.same_bits(ov.contiguous(), relu_out[with_res].contiguous()), "vs_bn_apply_mask output != vs_bn_apply output"
        assert R.untouched(obuf, olo[1], c)
        R.assert_mask(f"bn_apply_mask {tag} res={int(with_res)}", R.unpack_bits(bits, c), v64, delta, stored=ov.float())
    if not _pow2(c):
        return
    # RES_AFF: the residual is bf16(y2 * scale2 + shift2), formed in the kernel from a second unit's raw output
    sc2, sh2 = _vec(c, seed + 4, dev, "pos"), _vec(c, seed + 5, dev, 0.3)
    v64, hi, delta = R.bn_apply_ref(y, scale, shift, aff2=(res, sc2, sh2))
    bits = R.nan_filled((rows, c // 8), dev, torch.uint8)
    obuf, ov = _out(rows, c, dev, *olo)
    call("vs_bn_apply2", P(yv), P(scale), P(shift), P(rv), P(sc2), P(sh2), P(ov), P(bits), rows, c, yv.stride(0),
         rv.stride(0), ov.stride(0), S())
    R.assert_interval(f"bn_apply2 {tag}", ov, v64, delta, True, v64_hi=hi)
    assert R.untouched(obuf, olo[1], c)
    mask = R.unpack_bits(bits, c)
    assert torch.equal(mask, ov.float() > 0), "bn_apply2 mask bits differ from (stored output > 0)"
    amb = (v64 - delta <= 0) & (hi + delta >= 0)
    wrong = int(((mask != (v64 > 0)) & ~amb).sum())
    excl = float(amb.sum()) / amb.numel()
    print(f"PARITY bn_apply2 mask {tag} wrong={wrong} excl={excl:.2e}")
    assert wrong == 0 and excl <= R.EXCL_CAP


# ---------------------------------------------------------------------------------------------
# BN backward apply: vs_bn_bwd_apply, vs_bn_bwd_apply2
# ---------------------------------------------------------------------------------------------
def _bwd_operands(c, rows, seed, dev):
    d = dict(y=_randn((rows, c), seed, dev, 1.5, 0.3), dz=_randn((rows, c), seed + 1, dev),
             z=torch.relu(_randn((rows, c), seed + 2, dev)),
             mean=_vec(c, seed + 3, dev, 0.1) + 0.3, invstd=1.0 / (_vec(c, seed + 4, dev, "pos") + 0.5),
             gamma=_vec(c, seed + 5, dev, "pos"), beta=_vec(c, seed + 6, dev, 0.2),
             dgamma=_vec(c, seed + 7, dev, rows ** 0.5), dbeta=_vec(c, seed + 8, dev, rows ** 0.5))
    if _pow2(c):
        d["bits"] = torch.randint(0, 256, (rows, c // 8), generator=R.gen(seed + 9), dtype=torch.uint8).to(dev)
    return d


def _masked_grad(o, mask, c, tag):
    """-> (g64, elements whose mask decision is within delta of 0 | None) for MASK 0 .. 3."""
    g = o["dz"].double()
    if mask == 0:
        return g, None
    zero = torch.zeros((), dtype=torch.float64, device=g.device)  # (where, not a product: -x * 0 is -0)
    if mask == 1:
        return torch.where(o["z"].float() > 0, g, zero), None
    if mask == 3:
        return torch.where(R.unpack_bits(o["bits"], c), g, zero), None
    m64, dm = R.bn_mask_from_y(o["y"], o["mean"], o["invstd"], o["gamma"], o["beta"])
    amb = m64.abs() <= dm
    excl = float(amb.sum()) / amb.numel()
    print(f"PARITY mask-from-y {tag} excl={excl:.2e}")
    assert excl <= R.EXCL_CAP
    return torch.where(m64 > 0, g, zero), amb


BN_BWD_CASES = _edge_cases([8, 64, 2048, 4096]) + [(2048, 8193, False), (2048, 40000, False)] \
    + [(c, r, r == 7) for c in (72, 200) for r in (7, 1000)] + [(72, 60000, False)]


@pytest.mark.parametrize("c,rows,pitched", BN_BWD_CASES, ids=_ids(BN_BWD_CASES))
def test_bn_bwd_apply(c, rows, pitched, dev):
    """dy (and dres = the masked gradient, bit for bit) with dgamma / dbeta handed in.  Column-owner kernel: masks 0, 1
    (from z), 2 (recomputed from y), 3 (bits), each with and without dres, at the forward's C list and row edges plus
    nbatch 2 and the clamp; generic kernel <0>, <1>, <2> at C = 72 / 200 and at the stride-loop size.  Pitched cases:
    dz_ld, z_ld, y_ld, dy_ld and dres_ld all distinct, every byte outside the output slices untouched."""
    ops, call, P, S = _api()
    o = _bwd_operands(c, rows, 77 * c + rows, dev)
    lay = [(c + 8 * (i + 1), 8 * i) if pitched else (None, 0) for i in range(5)]  # dz, z, y, dy, dres
    _, dzv = _slice(o["dz"], *lay[0])
    _, zv = _slice(o["z"], *lay[1])
    _, yv = _slice(o["y"], *lay[2])
    tag0 = f"C{c} rows{rows}" + (" pitched" if pitched else "")
    for mask in ((0, 1, 2, 3) if _pow2(c) else (0, 1, 2)):
        tag = f"{tag0} mask{mask}"
        g64, amb = _masked_grad(o, mask, c, tag)
        v64, delta = R.bn_bwd_apply_ref(g64, o["y"], o["mean"], o["invstd"], o["gamma"], o["dgamma"], o["dbeta"], rows)
        zarg, z_ld, relu = (None, 0, 0) if mask == 0 else (zv, zv.stride(0), 1) if mask == 1 else (None, 0, 1) \
            if mask == 2 else (o["bits"], c // 8, 2)
        first = None
        for want_dres in (False, True):
            dybuf, dyv = _out(rows, c, dev, *lay[3])
            drbuf, drv = _out(rows, c, dev, *lay[4])
            call("vs_bn_bwd_apply", P(dzv), P(zarg), P(yv), P(o["mean"]), P(o["invstd"]), P(o["gamma"]),
                 P(o["beta"]) if mask == 2 else None, P(o["dgamma"]), P(o["dbeta"]), P(dyv), P(drv) if want_dres else None,
                 rows, c, dzv.stride(0), z_ld, yv.stride(0), dyv.stride(0), drv.stride(0) if want_dres else 0, relu, S())
            R.assert_interval(f"bn_bwd_apply {tag} dres={int(want_dres)}", dyv, v64, delta, exclude=amb)
            assert R.untouched(dybuf, lay[3][1], c), "bn_bwd_apply wrote dy outside its slice"
            if want_dres:
                want = g64.to(BF16)  # dz or 0: exact
                got = drv.contiguous()
                if amb is not None:
                    got, want = torch.where(amb, torch.zeros_like(got), got), torch.where(amb, torch.zeros_like(want), want)
                assert R.same_bits(got, want.contiguous()), f"dres {tag}: not the masked gradient bit for bit"
                assert R.untouched(drbuf, lay[4][1], c)
                assert R.same_bits(dyv.contiguous(), first), "dy changes with the DRES arm"
            else:
                assert R.untouched(drbuf, 0, 0), "dres written without being asked for"
                first = dyv.contiguous()
    if not _pow2(c):
        _refused(ops, "vs_bn_bwd_apply", P(dzv), P(zv), P(yv), P(o["mean"]), P(o["invstd"]), P(o["gamma"]), None,
                 P(o["dgamma"]), P(o["dbeta"]), P(first), None, rows, c, dzv.stride(0), c // 8, yv.stride(0), c, 0, 2, S())


@pytest.mark.parametrize("c,rows", [(64, 129), (2048, 5), (2048, 8193)])
def test_bn_bwd_apply2(c, rows, dev):
    """Two units fed by one masked gradient: both dy against two independent restatements, the two units' y / dy pitches
    all different, and bit for bit the one-unit kernel with the same bit mask."""
    ops, call, P, S = _api()
    a, b = _bwd_operands(c, rows, 5 * c + rows, dev), _bwd_operands(c, rows, 9 * c + rows + 100, dev)
    _, dzv = _slice(a["dz"], c + 8, 0)
    lds = [(c + 16, 8), (c + 24, 16), (c + 32, 24), (c + 40, 32)]  # ya, dya, yb, dyb
    _, yav = _slice(a["y"], *lds[0])
    _, ybv = _slice(b["y"], *lds[2])
    dabuf, dav = _out(rows, c, dev, *lds[1])
    dbbuf, dbv = _out(rows, c, dev, *lds[3])
    call("vs_bn_bwd_apply2", P(dzv), P(a["bits"]), P(yav), P(a["mean"]), P(a["invstd"]), P(a["gamma"]), P(a["dgamma"]),
         P(a["dbeta"]), P(dav), P(ybv), P(b["mean"]), P(b["invstd"]), P(b["gamma"]), P(b["dgamma"]), P(b["dbeta"]), P(dbv),
         rows, c, dzv.stride(0), yav.stride(0), dav.stride(0), ybv.stride(0), dbv.stride(0), S())
    g64, _ = _masked_grad(a, 3, c, "")
    for name, u, got, buf, lo in (("a", a, dav, dabuf, lds[1]), ("b", b, dbv, dbbuf, lds[3])):
        v64, delta = R.bn_bwd_apply_ref(g64, u["y"], u["mean"], u["invstd"], u["gamma"], u["dgamma"], u["dbeta"], rows)
        R.assert_interval(f"bn_bwd_apply2 C{c} rows{rows} unit {name}", got, v64, delta)
        assert R.untouched(buf, lo[1], c)
        _, one = _out(rows, c, dev)
        call("vs_bn_bwd_apply", P(dzv), P(a["bits"]), P(u["y"]), P(u["mean"]), P(u["invstd"]), P(u["gamma"]), None,
             P(u["dgamma"]), P(u["dbeta"]), P(one), None, rows, c, dzv.stride(0), c // 8, c, c, 0, 2, S())
        assert R.same_bits(got.contiguous(), one), "apply2 is not bitwise the one-unit pass"


# ---------------------------------------------------------------------------------------------
# BN backward reduce + finalize
# ---------------------------------------------------------------------------------------------
BN_RED_CASES = _edge_cases([8, 256, 2048, 4096]) + [(2048, 4097, False), (2048, 12289, False), (4096, 4097, False),
                                                     (256, 32769, False)]


@pytest.mark.parametrize("c,rows,pitched", BN_RED_CASES, ids=_ids(BN_RED_CASES))
def test_bn_bwd_reduce(c, rows, pitched, dev):
    """dbeta = sum g and dgamma = sum g xhat through vs_bn_bwd_reduce + the finalize, masks 0 .. 3, against fp64 sums
    of the same operands within (4 nbatch + log2 rl + 2 (+ 3)) * 2^-24 * sum |terms|.  C = 2048: rl = 1, no LDS tree;
    C = 4096: the tree's LDS is reused on the second column trip; rows = 1: every other row lane re-reads row 0, whose
    gradient is 64x larger here -- a kernel that counted a re-read row would miss by orders of magnitude; 4097 / 12289
    rows at C = 2048 and 32769 at C = 256 are the smallest with nbatch 2 / 4 / 2.  The partial buffer starts as NaN:
    every row of it must be written."""
    ops, call, P, S = _api()
    o = _bwd_operands(c, rows, 31 * c + rows, dev)
    o["dz"][0] *= 64.0
    lay = [(c + 8 * (i + 1), 8 * i) if pitched else (None, 0) for i in range(3)]
    _, dzv = _slice(o["dz"], *lay[0])
    _, zv = _slice(o["z"], *lay[1])
    _, yv = _slice(o["y"], *lay[2])
    nblk = int(ops._lib.load().vs_bn_bwd_reduce_rows(rows, c))
    nb, rl = R.bnb_batches(rows, c)
    assert nblk == -(-rows // (rl * 4 * nb))
    for mask in (0, 1, 2, 3):
        tag = f"C{c} rows{rows} nbatch{nb} mask{mask}" + (" pitched" if pitched else "")
        g64, amb = _masked_grad(o, mask, c, tag)
        zarg, z_ld, relu = (None, 0, 0) if mask == 0 else (zv, zv.stride(0), 1) if mask == 1 else (None, 0, 1) \
            if mask == 2 else (o["bits"], c // 8, 2)
        partial = R.nan_filled((nblk, 2, c), dev, torch.float32)
        dgamma, dbeta = R.nan_filled((c,), dev, torch.float32), R.nan_filled((c,), dev, torch.float32)
        call("vs_bn_bwd_reduce", P(dzv), P(zarg), P(yv), P(o["mean"]), P(o["invstd"]), P(o["gamma"]) if mask == 2 else None,
             P(o["beta"]) if mask == 2 else None, P(partial), rows, c, dzv.stride(0), z_ld, yv.stride(0), relu, S())
        ops._bn_bwd_finalize(partial, nblk, dgamma, dbeta, c)
        db64, bb, dg64, bg = R.bn_bwd_sums_ref(g64, o["y"], o["mean"], o["invstd"], rows, c, uncertain=amb)
        R.assert_sum(f"bn_bwd_reduce dbeta {tag}", dbeta, db64, bb)
        R.assert_sum(f"bn_bwd_reduce dgamma {tag}", dgamma, dg64, bg)


def test_bn_bwd_reduce_refuses_other_channel_counts(dev):
    ops, call, P, S = _api()
    assert int(ops._lib.load().vs_bn_bwd_reduce_rows(100, 72)) == -1
    o = _bwd_operands(72, 16, 3, dev)
    partial = torch.zeros(4, 2, 72, device=dev)
    _refused(ops, "vs_bn_bwd_reduce", P(o["dz"]), None, P(o["y"]), P(o["mean"]), P(o["invstd"]), None, None, P(partial), 16,
             72, 72, 0, 72, 0, S())


# ---------------------------------------------------------------------------------------------
# helpers for the 5-D (NCDHW logical, channels-last memory) pool tests
# ---------------------------------------------------------------------------------------------
def _act(x, dev, ld=None, off=0):
    """NCDHW cpu tensor -> (buffer [N,T,H,W,ld], bf16 activation view) on the GPU, NaN pattern outside the slice."""
    n, c, t, h, w = x.shape
    buf = R.nan_filled((n, t, h, w, ld or c), dev)
    v = buf.permute(0, 4, 1, 2, 3)[:, off:off + c]
    v.copy_(x.to(dev))
    return buf, v


def _out_act(n, c, t, h, w, dev, ld=None, off=0):
    buf = R.nan_filled((n, t, h, w, ld or c), dev)
    return buf, buf.permute(0, 4, 1, 2, 3)[:, off:off + c]


def _cl(v):
    """activation / NCDHW tensor -> dense [N*T, H, W, C]."""
    n, c, t, h, w = v.shape
    return v.permute(0, 2, 3, 4, 1).reshape(n * t, h, w, c)


def _grad_like(shape, seed):
    """bf16 gradients with |value| in [0.25, 4): the pool backward's fp32 sums are then exact (maxpool_hw_bwd_delta)."""
    g = R.gen(seed)
    mag = torch.rand(shape, generator=g) * 3.75 + 0.25
    sign = (torch.rand(shape, generator=g) > 0.5).float() * 2 - 1
    return (mag * sign).to(BF16)


def _check_maxpool_hw(x, dev, tag, pitched=False, seed=0):
    """x: NCDHW bf16 on the CPU.  Forward (with and without idx) bit for bit against torch, backward against the fp64
    sum by torch's argmax."""
    ops, _, _, _ = _api()
    n, c, t, h, w = x.shape
    yr, tapr = R.maxpool_hw_ref(x)
    ho, wo = yr.shape[3], yr.shape[4]
    _, xv = _act(x, dev, *((c + 16, 8) if pitched else (None, 0)))
    ybuf, yv = _out_act(n, c, t, ho, wo, dev, *((c + 8, 0) if pitched else (None, 0)))
    y, idx = ops.maxpool_hw(xv, out=yv, want_idx=True)
    assert R.same_bits(_cl(y).cpu(), _cl(yr)), f"maxpool_hw {tag}: values differ from torch"
    assert torch.equal(idx.cpu().reshape(n * t, ho, wo, c), _cl(tapr)), f"maxpool_hw {tag}: argmax differs from torch"
    assert R.untouched(ybuf, 0, c)
    y2, none = ops.maxpool_hw(xv, want_idx=False)
    assert none is None and R.same_bits(_cl(y2), _cl(y))
    dy = _grad_like(tuple(yr.shape), seed + 1)
    _, dyv = _act(dy, dev, *((c + 24, 16) if pitched else (None, 0)))
    dx = ops.maxpool_hw_bwd(dyv, idx, (n, c, t, h, w))
    dx64, ab = R.maxpool_hw_bwd_ref(_cl(dy), _cl(tapr), h, w)
    R.assert_interval(f"maxpool_hw_bwd {tag}", _cl(dx).cpu(), dx64, R.maxpool_hw_bwd_delta(dy, ab))
    return y, idx


# ---------------------------------------------------------------------------------------------
# the stems' fused passes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n,t,h,w", [(8, 2, 3, 16, 16), (64, 2, 2, 14, 18), (16, 1, 1, 7, 9), (64, 1, 2, 112, 112),
                                       (8, 2, 2, 1, 5), (8, 1, 2, 2, 2), (16, 2, 1, 6, 1), (8, 1, 1, 1, 1), (8, 1, 3, 2, 7)])
def test_stem_fused_passes_and_the_chain_they_replace(c, n, t, h, w, dev):
    """The unfused chain bn_apply -> maxpool_hw and maxpool_hw_bwd -> bn_bwd (mask recomputed from y) against fp64 /
    torch pass by pass, and the fused launches bit for bit against it: the bitwise pair of test_gpu_bn_pool.py anchored
    to something other than each other, plus H or W of 1 and 2."""
    ops, _, _, _ = _api()
    seed = 13 * c + 100 * h + w
    rows = n * t * h * w
    x = (torch.randn(n, c, t, h, w, generator=R.gen(seed)) * 1.5 + 0.3).to(BF16)
    _, y = _act(x, dev)
    scale, shift = _vec(c, seed + 1, dev, "pos"), _vec(c, seed + 2, dev, 0.3)
    tag = f"stem C{c} {n}x{t}x{h}x{w}"
    z = ops.bn_apply(y, scale, shift, None, True)
    y2d = _cl(y).reshape(rows, c)
    v64, _, delta = R.bn_apply_ref(y2d, scale, shift)
    R.assert_interval(f"bn_apply {tag}", _cl(z).reshape(rows, c), v64, delta, True)
    p_ref, i_ref = _check_maxpool_hw(z.cpu(), dev, tag, seed=seed)
    p, i = ops.bn_apply_maxpool(y, scale, shift)
    assert R.same_bits(_cl(p), _cl(p_ref)) and torch.equal(i, i_ref.reshape(i.shape)), "fused forward != unfused"
    mean, invstd = _vec(c, seed + 3, dev, 0.1) + 0.3, 1.0 / (_vec(c, seed + 4, dev, "pos") + 0.5)
    gamma, beta = _vec(c, seed + 5, dev, "pos"), _vec(c, seed + 6, dev, 0.3)
    _, dp = _act(_grad_like(tuple(p.shape), seed + 7), dev)
    dz = ops.maxpool_hw_bwd(dp, i_ref, tuple(y.shape))
    dy_ref, _, dg_ref, db_ref = ops.bn_bwd(dz, None, y, mean, invstd, gamma, True, False, beta=beta)
    o = dict(dz=_cl(dz).reshape(rows, c), y=y2d, mean=mean, invstd=invstd, gamma=gamma, beta=beta)
    g64, amb = _masked_grad(o, 2, c, tag)
    db64, bb, dg64, bg = R.bn_bwd_sums_ref(g64, y2d, mean, invstd, rows, c, uncertain=amb)
    R.assert_sum(f"bn_bwd dbeta {tag}", db_ref, db64, bb)
    R.assert_sum(f"bn_bwd dgamma {tag}", dg_ref, dg64, bg)
    v64, delta = R.bn_bwd_apply_ref(g64, y2d, mean, invstd, gamma, dg_ref, db_ref, rows)
    R.assert_interval(f"bn_bwd dy {tag}", _cl(dy_ref).reshape(rows, c), v64, delta, exclude=amb)
    dy, _, dg, db = ops.bn_bwd(None, None, y, mean, invstd, gamma, True, False, beta=beta, pool_src=(dp, i_ref))
    assert R.same_bits(_cl(dy), _cl(dy_ref)) and torch.equal(dg, dg_ref) and torch.equal(db, db_ref), "fused backward != unfused"


# ---------------------------------------------------------------------------------------------
# maxpool_hw (3x3, stride 2, pad 1)
# ---------------------------------------------------------------------------------------------
HW_CASES = [(8, 2, 1, 1, False), (8, 2, 1, 8, False), (8, 1, 2, 2, False), (72, 2, 3, 7, False), (8, 2, 7, 3, True),
            (72, 1, 8, 8, True), (8, 2, 7, 7, False), (8, 1, 8, 2, False), (72, 1, 2, 1, False), (8, 1, 3, 3, True),
            (72, 3, 7, 8, False)]


@pytest.mark.parametrize("c,t,h,w,pitched", HW_CASES, ids=[f"C{c}_T{t}_{h}x{w}" + ("_pitched" if p else "")
                                                           for c, t, h, w, p in HW_CASES])
def test_maxpool_hw(c, t, h, w, pitched, dev):
    """H, W in {1, 2, 3, 7, 8}: every window clipped / one window / odd and even edges; C = 8 and 72; inputs pass
    through ReLU, so exact ties at 0 are frequent and the first maximum in scan order must win; pitched input, output and
    gradient; idx = None."""
    x = torch.relu(torch.randn(2, c, t, h, w, generator=R.gen(17 * c + 10 * h + w))).to(BF16)
    _check_maxpool_hw(x, dev, f"C{c} 2x{t}x{h}x{w}" + (" pitched" if pitched else ""), pitched, seed=c + h)


def test_maxpool_hw_nan_and_neg_inf_at_every_tap(dev):
    """Plane p < 9: a NaN at tap p of the full window (1, 1) and a -inf at tap p of the full window (2, 2); planes 18 .. 21:
    a NaN at each of the four in-image taps of the corner window (0, 0) and a -inf at each of the four of the clipped
    window (3, 3) of a 7 x 7 map.  One plant per window: value and argmax follow torch (NaN wins and names its tap, -inf
    never wins)."""
    g = R.gen(5)
    x = torch.randn(2, 8, 11, 7, 7, generator=g).to(BF16)
    def plane(p):  # a view [C, 7, 7]: plane p = n * 11 + t
        return x[p // 11, :, p % 11]

    for p in range(9):
        dh, dw = divmod(p, 3)
        plane(p)[:, 1 + dh, 1 + dw] = float("nan")
        plane(9 + p)[:, 3 + dh, 3 + dw] = float("-inf")
    for q in range(4):
        plane(18 + q)[:, q >> 1, q & 1] = float("nan")
        plane(18 + q)[:, 5 + (q >> 1), 5 + (q & 1)] = float("-inf")
    assert int(torch.isnan(x).sum()) == 13 * 8
    y, _ = _check_maxpool_hw(x, dev, "nan/-inf 22 planes of 7x7")
    assert int(torch.isnan(y).sum()) > 13 * 8  # a NaN reaches every window it lies in


@pytest.mark.parametrize("nt", [(1 << 20) - 1, 1 << 20], ids=["below_2p24", "at_2p24"])
def test_maxpool_hw_fwd_index_arms(nt, dev):
    """nt x 4 x 4 x (C/8 = 1) output chunks: one fewer than 2^24 (the float-reciprocal index split at its upper limit) and
    2^24 (the 64-bit arm).  y against torch.max_pool3d of the same device tensor; argmax = the first tap equal to y."""
    ops, _, _, _ = _api()
    x = torch.relu(_randn((1, nt, 8, 8, 8), nt, dev))  # [N=1, T=nt, H, W, C]
    xv = x.permute(0, 4, 1, 2, 3)
    y, idx = ops.maxpool_hw(xv, want_idx=True)
    want = torch.nn.functional.max_pool3d(xv, (1, 3, 3), (1, 2, 2), (0, 1, 1))
    assert torch.equal(_cl(y), _cl(want))
    assert torch.equal(idx.reshape(nt, 4, 4, 8), R.first_max_tap(x[0], _cl(y)))


@pytest.mark.parametrize("nt", [(1 << 18) - 1, 1 << 18], ids=["below_2p24", "at_2p24"])
def test_maxpool_hw_bwd_index_arms(nt, dev):
    """nt x 8 x 8 x (C/8 = 1) input chunks, one fewer than 2^24 and 2^24 (64-bit arm of the backward).  The argmax bytes
    are validated (first tap equal to y, y = torch's max), then dx against the fp64 sum of dy by those bytes."""
    ops, _, _, _ = _api()
    x = torch.relu(_randn((1, nt, 8, 8, 8), nt + 7, dev))
    xv = x.permute(0, 4, 1, 2, 3)
    y, idx = ops.maxpool_hw(xv, want_idx=True)
    assert torch.equal(_cl(y), _cl(torch.nn.functional.max_pool3d(xv, (1, 3, 3), (1, 2, 2), (0, 1, 1))))
    idx4 = idx.reshape(nt, 4, 4, 8)
    assert torch.equal(idx4, R.first_max_tap(x[0], _cl(y)))
    gdev = torch.Generator(device=dev).manual_seed(nt)
    mag = torch.rand((1, nt, 4, 4, 8), device=dev, generator=gdev) * 3.75 + 0.25
    dy = (mag * ((torch.rand((1, nt, 4, 4, 8), device=dev, generator=gdev) > 0.5).float() * 2 - 1)).to(BF16)
    dx = ops.maxpool_hw_bwd(dy.permute(0, 4, 1, 2, 3), idx, (1, 8, nt, 8, 8))
    dx64, ab = R.maxpool_hw_bwd_ref(dy[0], idx4, 8, 8)
    R.assert_interval(f"maxpool_hw_bwd nt={nt} 8x8 C8", _cl(dx), dx64, R.maxpool_hw_bwd_delta(dy, ab))


# ---------------------------------------------------------------------------------------------
# maxpool_t, maxpool_hw2
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt,c,t,h,w", [(1, 8, 3, 3, 3), (2, 72, 4, 5, 3), (4, 8, 8, 2, 3), (2, 1024, 8, 28, 28)],
                         ids=["kt1", "kt2_C72", "kt4", "kt2_stride_loop"])
def test_maxpool_t(kt, c, t, h, w, dev):
    """kt = 1, 2, 4 with ties (ReLU) and a planted NaN (first, middle and last slot of a window); 2 x 4 x 784 x 128 chunks
    wrap the capped grid.  Values, argmax and the backward (a copy or 0) bit for bit against torch."""
    ops, _, _, _ = _api()
    x = torch.relu(_randn((2, c, t, h, w), kt + c, dev)).cpu()
    for d in range(kt):
        x[d % 2, d % c, d, 0, d % w] = float("nan")  # window 0 of position (0, d % w), slot d
    yr, ir = R.maxpool_t_ref(x, kt)
    _, xv = _act(x, dev)
    y, idx = ops.maxpool_t(xv, kt, want_idx=True)
    assert R.same_bits(_cl(y).cpu(), _cl(yr)) and int(torch.isnan(yr).sum()) == kt
    assert torch.equal(idx.cpu().reshape(_cl(ir).shape), _cl(ir))
    dy = _grad_like(tuple(yr.shape), kt)
    _, dyv = _act(dy, dev)
    dx = ops.maxpool_t_bwd(dyv, idx, tuple(x.shape), kt)
    want = torch.where(torch.arange(t).view(1, 1, t, 1, 1) % kt == ir.long().repeat_interleave(kt, dim=2),
                       dy.repeat_interleave(kt, dim=2), torch.zeros((), dtype=BF16))
    assert R.same_bits(_cl(dx).cpu(), _cl(want))


@pytest.mark.parametrize("c,t,h,w", [(8, 2, 2, 2), (72, 1, 5, 7), (8, 3, 6, 10), (72, 2, 3, 2), (8, 1, 7, 7)])
def test_maxpool_hw2(c, t, h, w, dev):
    """2x2 stride 2: odd H and W (the dropped last row / column get exact zeros in dx), H = W = 2, C = 8 and 72, ties."""
    ops, _, _, _ = _api()
    x = torch.relu(torch.randn(2, c, t, h, w, generator=R.gen(c + h * w))).to(BF16)
    yr, ir = R.maxpool_hw2_ref(x)
    _, xv = _act(x, dev)
    y, idx = ops.maxpool_hw2(xv)
    assert R.same_bits(_cl(y).cpu(), _cl(yr))
    assert torch.equal(idx.cpu().reshape(_cl(ir).shape), _cl(ir))
    dy = _grad_like(tuple(yr.shape), c)
    _, dyv = _act(dy, dev)
    dx = ops.maxpool_hw2_bwd(dyv, idx, tuple(x.shape)).cpu()
    xr = x.float().requires_grad_(True)
    torch.nn.functional.max_pool3d(xr, (1, 2, 2), (1, 2, 2)).backward(dy.float())
    assert R.same_bits(dx.float(), xr.grad)
    assert float(dx[..., 2 * (h // 2):, :].float().abs().sum()) == 0 and float(dx[..., 2 * (w // 2):].float().abs().sum()) == 0


@pytest.mark.parametrize("q", [0, 1, 2, 3])
def test_maxpool_hw2_nan_at_each_window_position(q, dev):
    """torch.nn.functional.max_pool3d (what the reference's Nonlocal pool calls) returns NaN, and the NaN's position,
    wherever in the 2x2 window the NaN sits; a pool that kept `v > best` alone would drop a NaN at positions 1 .. 3 and
    hide a diverged activation from the loss."""
    ops, _, _, _ = _api()
    x = torch.randn(2, 16, 2, 4, 6, generator=R.gen(40 + q)).to(BF16)
    x[0, :, 0, q >> 1, q & 1] = float("nan")  # window (0, 0)
    x[1, 3, 1, 2 + (q >> 1), 4 + (q & 1)] = float("nan")  # window (1, 2), one channel
    x[1, 5, 0, (q >> 1), 2 + (q & 1)] = float("-inf")
    yr, ir = R.maxpool_hw2_ref(x)
    assert int(torch.isnan(yr).sum()) == 17
    _, xv = _act(x, dev)
    y, idx = ops.maxpool_hw2(xv)
    assert R.same_bits(_cl(y).cpu(), _cl(yr)), f"a NaN at window position {q} does not reach the pooled tensor"
    assert torch.equal(idx.cpu().reshape(_cl(ir).shape), _cl(ir))


# ---------------------------------------------------------------------------------------------
# global average pool
# ---------------------------------------------------------------------------------------------
AVG_CASES = [(1, 8), (18, 256), (32, 264), (33, 2304), (72, 8), (97, 264), (128, 256), (129, 2304), (392, 264), (392, 2304)]


@pytest.mark.parametrize("rows,c", AVG_CASES, ids=[f"rows{r}_C{c}" for r, c in AVG_CASES])
def test_avgpool(rows, c, dev):
    """rows per clip around the 4-in-flight loop (needs r + 96 < rows: 97 is the first size with a trip, 128 / 129 the
    lane edge, 392 the workload's) and the tail; C/8 = 1, 32, 33, 288 (the last block's clamped columns); x_ld > C; a
    non-zero c_off into a wider fp32 out whose other columns stay NaN; the backward into a pitched dx."""
    ops, call, P, S = _api()
    n, ld, ctot, c_off = 3, c + 16, c + 40, 24
    x = _randn((n * rows, c), rows * 7 + c, dev, 1.0, 0.5)
    _, xv = _slice(x, ld, 8)
    out = R.nan_filled((n, ctot), dev, torch.float32)
    call("vs_avgpool_fwd", P(xv), P(out), n, rows, c, ld, ctot, c_off, S())
    ref, bound = R.avgpool_ref(x.view(n, rows, c), rows)
    R.assert_sum(f"avgpool_fwd rows{rows} C{c}", out[:, c_off:c_off + c], ref, bound)
    assert R.untouched(out, c_off, c), "avgpool_fwd wrote outside its columns of the concat"
    dout = torch.randn(n, ctot, generator=R.gen(rows + c)).to(dev)
    dxbuf, dxv = _out(n * rows, c, dev, ld, 8)
    call("vs_avgpool_bwd", P(dout), P(dxv), n, rows, c, ld, ctot, c_off, S())
    v64 = (dout[:, c_off:c_off + c].double() / rows).view(n, 1, c).expand(n, rows, c).reshape(n * rows, c)
    R.assert_interval(f"avgpool_bwd rows{rows} C{c}", dxv, v64, 2.0 ** -23 * v64.abs())
    assert R.untouched(dxbuf, 8, c)


# ---------------------------------------------------------------------------------------------
# fp32 residual stream
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,rows", [(8, 37), (72, 37), (2048, 5), (72, 60000)])
def test_residual_add_f32(c, rows, dev):
    """out32 = relu?(res + branch) is ONE fp32 add: bit for bit torch's; out16 = bf16(out32) bit for bit.  fp32 and bf16
    residual arms, with and without ReLU, every pitch different, 60 000 x 9 chunks wrap the capped grid."""
    ops, call, P, S = _api()
    br = _randn((rows, c), c + rows, dev)
    r16 = _randn((rows, c), c + rows + 1, dev)
    r32 = _randn((rows, c), c + rows + 2, dev, dtype=torch.float32)
    _, bv = _slice(br, c + 8, 8)
    for f32 in (True, False):
        _, rv = _slice(r32 if f32 else r16, c + 16, 8)
        for relu in (0, 1):
            o32buf, o32 = _out(rows, c, dev, c + 4, 4, torch.float32)
            o16buf, o16 = _out(rows, c, dev, c + 24, 16)
            call("vs_residual_add_f32", P(bv), P(rv) if f32 else None, None if f32 else P(rv), P(o32), P(o16), rows, c,
                 c + 8, c + 16, c + 4, c + 24, relu, S())
            want = br.float() + (r32 if f32 else r16.float())
            if relu:
                want = torch.relu(want)
            assert R.same_bits(o32.contiguous(), want), f"out32 C{c} f32={f32} relu={relu}"
            assert R.same_bits(o16.contiguous(), want.to(BF16)), f"out16 C{c} f32={f32} relu={relu}"
            assert R.untouched(o32buf, 4, c) and R.untouched(o16buf, 16, c)


# ---------------------------------------------------------------------------------------------
# row softmax, its backward, bf16 column sum
# ---------------------------------------------------------------------------------------------
SOFTMAX_CASES = [(4, 1), (252, 4), (256, 5), (260, 37), (1568, 37), (4092, 5), (4096, 4)]


def _softmax_scores(p, rows):
    s = (torch.randn(rows, p, generator=R.gen(p + rows)) * 3).to(BF16)
    s[0, :] = -60.0
    s[0, p // 2] = 60.0  # a dominant entry: every other probability underflows
    if rows > 1:
        s[1, :] = 1.5  # a constant row: exactly 1 / P
    return s


@pytest.mark.parametrize("p,rows", SOFTMAX_CASES, ids=[f"P{p}_rows{r}" for p, r in SOFTMAX_CASES])
def test_softmax_rows(p, rows, dev):
    """P = 4, 252 / 256 / 260 (one 8-byte piece per lane and its edges), 1568, 4092 / 4096 (all 16 pieces); rows = 1, 4,
    5, 37 (four rows per block); in place and out of place agree bit for bit.  delta = 16 e32 max |v64| of the row
    (docs/gpt2_ops_parity.md's margin): elements far below their row's maximum are ambiguous under it by construction,
    so the 1 % cap of the arithmetic kernels is not asserted here; the share is printed."""
    ops, _, _, _ = _api()
    s = _softmax_scores(p, rows)
    ref64, ref32 = R.softmax_ref(s, torch.float64), R.softmax_ref(s, torch.float32)
    delta, e32 = R.softmax_delta(ref64, ref32)
    sd = s.to(dev)
    out = R.nan_filled((rows + 1, p), dev)
    ops.softmax_rows_bf16(sd, rows, p, out=out)
    inplace = ops.softmax_rows_bf16(sd.clone(), rows, p)
    assert R.same_bits(out[:rows], inplace) and R.untouched(out[rows:], 0, 0)
    err = float((inplace.cpu().double() - R.bf16_rne(ref64)).abs().max() / ref64.abs().max())
    print(f"PARITY softmax_rows P{p} rows{rows} e32={e32:.3e} err_vs_rne={err:.3e}")
    R.assert_interval(f"softmax_rows P{p} rows{rows}", inplace.cpu(), ref64, delta, amb_cap=None)
    assert float(inplace[0, p // 2]) == 1.0 and float(inplace[0].float().sum()) == 1.0


@pytest.mark.parametrize("p,rows", SOFTMAX_CASES, ids=[f"P{p}_rows{r}" for p, r in SOFTMAX_CASES])
def test_softmax_rows_bwd(p, rows, dev):
    """ds = scale p (dp - sum dp p) at the forward's shapes, p the bf16 probabilities (row 0 one-hot: ds = 0 exactly)."""
    ops, _, _, _ = _api()
    prob = R.softmax_ref(_softmax_scores(p, rows), torch.float32).to(BF16)
    dp = torch.randn(rows, p, generator=R.gen(p * rows + 1)).to(BF16)
    ref64, ref32 = R.softmax_bwd_ref(prob, dp, 0.25, torch.float64), R.softmax_bwd_ref(prob, dp, 0.25, torch.float32)
    delta, e32 = R.softmax_delta(ref64, ref32)
    pd, dpd = prob.to(dev), dp.to(dev)
    out = R.nan_filled((rows + 1, p), dev)
    ops.softmax_rows_bwd_bf16(pd, dpd, rows, p, 0.25, out=out)
    inplace = ops.softmax_rows_bwd_bf16(pd, dpd.clone(), rows, p, 0.25)
    assert R.same_bits(out[:rows], inplace) and R.untouched(out[rows:], 0, 0)
    err = float((inplace.cpu().double() - R.bf16_rne(ref64)).abs().max() / (float(ref64.abs().max()) or 1.0))
    print(f"PARITY softmax_rows_bwd P{p} rows{rows} e32={e32:.3e} err_vs_rne={err:.3e}")
    R.assert_interval(f"softmax_rows_bwd P{p} rows{rows}", inplace.cpu(), ref64, delta, amb_cap=None)


def test_softmax_rows_refuses_unsupported_widths(dev):
    ops, call, P, S = _api()
    x = torch.zeros(4, 4104, dtype=BF16, device=dev)
    for p in (4100, 6):
        _refused(ops, "vs_softmax_rows_bf16", P(x), P(x), 4, p, S())
        _refused(ops, "vs_softmax_rows_bwd_bf16", P(x), P(x), P(x), 4, p, 0.25, S())


COLSUM_CASES = [(1, 64, 64), (16, 1, 8), (17, 100, 104), (112, 64, 64), (113, 130, 136), (129, 64, 72), (241, 100, 100),
                (241, 130, 144)]


@pytest.mark.parametrize("rows,c,ld", COLSUM_CASES, ids=[f"{r}x{c}_ld{ld}" for r, c, ld in COLSUM_CASES])
def test_colsum_bf16(rows, c, ld, dev):
    """Tail loop only (rows <= 112), the 8-in-flight loop from its first size (113), every wave in it plus a tail row
    (129), a second trip (241); C = 1, 64, 100, 130 (clamped lanes, three blocks); ld > C with NaN beside the columns."""
    ops, call, P, S = _api()
    x = _randn((rows, c), rows * 3 + c, dev, 1.0, 0.25)
    _, xv = _slice(x, ld if ld > c else None, 0)
    out = R.nan_filled((1, c + 8), dev, torch.float32)
    call("vs_colsum_bf16", P(xv), P(out), rows, c, ld, S())
    ref, bound = R.colsum_ref(x, rows)
    R.assert_sum(f"colsum_bf16 {rows}x{c} ld{ld}", out[0, :c], ref, bound)
    assert R.untouched(out, 0, c)
