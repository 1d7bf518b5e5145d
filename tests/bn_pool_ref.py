"""fp64 restatements of the kernels of csrc/bn_pool.hip and the acceptance criteria of their tests
(docs/bn_pool_parity.md holds the derivations and the measured figures).  Device agnostic: every function
computes where its operands live, so tests/test_bn_pool_ref.py runs the same code on the CPU.

Every bound is derived by counting the fp32 roundings of the kernel's source; none is fitted to an output.

  1. bf16 outputs of elementwise arithmetic: with v64 the fp64 value and delta >= |v32 - v64|, a stored element must
     satisfy bf16(v64 - delta) <= got <= bf16(v64 + delta) (round to nearest even): the exact rounding except within
     delta of a tie.  At most AMB_CAP of a case's elements may have two admissible values.
  2. ReLU decisions: equal to v64 > 0 wherever |v64| > delta; at most EXCL_CAP of the elements may be closer to 0.
  3. selections and copies: bit for bit (no helper needed beyond `same_bits`).
  4. fp32 sums: |got - fp64 sum| <= (longest sequential chain + tree depth) * 2^-24 * sum |terms|.
  5. row softmax: delta = 16 * e32 * max |v64| of the row, e32 the error of the fp32 torch restatement.
"""
import math

import torch

BF16 = torch.bfloat16
U32 = 2.0 ** -24  # one fp32 rounding, relative to the rounded quantity
AMB_CAP = 0.01  # share of elements whose interval holds two bf16 values
EXCL_CAP = 0.001  # share of elements whose ReLU decision is within delta of 0
SOFTMAX_FACTOR = 16.0  # docs/gpt2_ops_parity.md
NAN_PATTERN = 0x7FC1  # a quiet bf16 NaN no kernel here produces (the canonical one is 0x7FC0)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rb(x):
    """bf16 rounding (the operands the kernels read), kept as bf16."""
    return x.to(BF16)


def bf16_rne(v64):
    """fp64 -> nearest bf16 (ties to even) in ONE rounding, returned as fp64.  (`.to(bfloat16)` of a double rounds to
    fp32 first.)  Normal range only: every value here is far from bf16's exponent limits, 0 stays 0."""
    assert v64.dtype == torch.float64
    b = v64.contiguous().view(torch.int64)
    lsb = (b >> 45) & 1
    b = (b + ((1 << 44) - 1) + lsb) & ~((1 << 45) - 1)
    return b.view(torch.float64)


def bf16_trunc(v32):
    """fp32 -> bf16 by dropping the low 16 bits: the error class the interval criterion exists to reject."""
    assert v32.dtype == torch.float32
    return (v32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)


def nan_filled(shape, device, dtype=BF16):
    """A buffer holding NAN_PATTERN (bf16) / NaN (fp32) / 0xA5 (uint8) everywhere: what a kernel must leave alone."""
    if dtype == BF16:
        return torch.full(shape, NAN_PATTERN, dtype=torch.int16, device=device).view(BF16)
    if dtype == torch.uint8:
        return torch.full(shape, 0xA5, dtype=torch.uint8, device=device)
    return torch.full(shape, float("nan"), dtype=dtype, device=device)


def untouched(buf, c_off, c):
    """Every element of the 2-D (rows x pitch) view of `buf` outside columns [c_off, c_off + c) still holds the pattern."""
    b = buf.reshape(-1, buf.shape[-1])
    if b.dtype == BF16:
        b = b.view(torch.int16)
        ok = b == NAN_PATTERN
    elif b.dtype == torch.uint8:
        ok = b == 0xA5
    else:
        ok = torch.isnan(b)
    return bool(ok[:, :c_off].all()) and bool(ok[:, c_off + c:].all())


def same_bits(a, b):
    """Bitwise equality of two tensors of one dtype (any NaN counts as equal to any NaN of the same sign bit)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        na, nb = torch.isnan(a), torch.isnan(b)
        if not torch.equal(na, nb):
            return False
        a, b = torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b)
        if a.dtype == BF16:
            return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))
        if a.dtype == torch.float32:
            return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def unpack_bits(bits, c):
    """uint8 [rows, C/8] (bit e of byte cb: channel 8 cb + e) -> bool [rows, C]."""
    sh = torch.arange(8, device=bits.device, dtype=torch.uint8)
    return ((bits.unsqueeze(-1) >> sh) & 1).bool().reshape(bits.shape[0], c)


def pack_bits(mask):
    rows, c = mask.shape
    sh = torch.arange(8, device=mask.device, dtype=torch.int32)
    return (mask.reshape(rows, c // 8, 8).to(torch.int32) << sh).sum(-1).to(torch.uint8)


# ---------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------
def interval_stats(got, v64, delta, relu=False, v64_hi=None, exclude=None):
    """Criterion 1.  `v64_hi`: upper end of the exact value where it has two admissible values itself (RES_AFF's inner
    rounding); `exclude`: elements left out (an ambiguous ReLU decision feeding them), counted in `excl`.
    -> bad: elements outside their interval; amb: share with two admissible values; off_rne: share whose stored value is
    not bf16(v64) itself (|got - v64| / delta is dominated by the bf16 rounding and says nothing about the kernel)."""
    lo_v, hi_v = v64 - delta, (v64 if v64_hi is None else v64_hi) + delta
    if relu:
        lo_v, hi_v = lo_v.clamp_min(0.0), hi_v.clamp_min(0.0)
    lo, hi = bf16_rne(lo_v), bf16_rne(hi_v)
    g = got.double()
    bad = ~((g >= lo) & (g <= hi))
    n = max(g.numel(), 1)
    excl = 0.0
    if exclude is not None:
        bad = bad & ~exclude
        excl = float(exclude.sum()) / n
    centre = bf16_rne(v64.clamp_min(0.0) if relu else v64)
    return dict(bad=int(bad.sum()), amb=float((lo != hi).sum()) / n, excl=excl,
                off_rne=float((g != centre).sum()) / n, n=g.numel())


def assert_interval(name, got, v64, delta, relu=False, v64_hi=None, exclude=None, amb_cap=AMB_CAP):
    s = interval_stats(got, v64, delta, relu, v64_hi, exclude)
    print(f"PARITY {name} n={s['n']} outside={s['bad']} off_rne={s['off_rne']:.2e} amb={s['amb']:.2e} "
          f"excl={s['excl']:.2e}")
    assert s["bad"] == 0, f"{name}: {s['bad']} of {s['n']} elements outside [bf16(v64 - d), bf16(v64 + d)]"
    if amb_cap is not None:
        assert s["amb"] <= amb_cap, f"{name}: ambiguous share {s['amb']:.3e} above {amb_cap}"
    assert s["excl"] <= EXCL_CAP, f"{name}: excluded share {s['excl']:.3e} above {EXCL_CAP}"
    return s


def assert_mask(name, mask, v64, delta, stored=None):
    """Criterion 2.  mask (bool) == (v64 > 0) wherever |v64| > delta; == (stored > 0) everywhere.  -> excluded elements."""
    amb = v64.abs() <= delta
    n = max(mask.numel(), 1)
    bad = int(((mask != (v64 > 0)) & ~amb).sum())
    excl = float(amb.sum()) / n
    print(f"PARITY {name} n={mask.numel()} wrong={bad} excl={excl:.2e}")
    assert bad == 0, f"{name}: {bad} ReLU decisions differ from v64 > 0 outside delta"
    assert excl <= EXCL_CAP, f"{name}: {excl:.3e} of the decisions lie within delta of 0"
    if stored is not None:
        assert torch.equal(mask, stored > 0), f"{name}: mask bits differ from (stored output > 0)"
    return amb


def assert_sum(name, got, ref64, bound):
    """Criterion 4: |got - ref64| <= bound elementwise (bound 0: exact)."""
    err = (got.double() - ref64).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf),
                                                                             torch.zeros_like(err)))
    r = float(ratio.max()) if ratio.numel() else 0.0
    print(f"PARITY {name} n={got.numel()} err/bound={r:.3f}")
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite sum"
    assert r <= 1.0, f"{name}: error {r:.3f} x the derived bound"
    return r


# ---------------------------------------------------------------------------------------------
# restatements.  Activations are [rows, C] views (any row pitch); per-channel parameters fp32 [C].
# ---------------------------------------------------------------------------------------------
def bn_apply_ref(y, scale, shift, res=None, aff2=None):
    """v = y * scale + shift (+ res | + bf16(y2 * scale2 + shift2)) before the ReLU.  -> (v64, v64_hi | None, delta).
    delta = 2^-22 * (|y scale| + |shift| + |res|): fma + add are 2 roundings of at most 2^-24 of that sum each, the
    generic kernel may round the product separately (3); 4 * 2^-24 covers both.  aff2 = (y2, scale2, shift2): the
    inner value is rounded to bf16 once; where it lies within 2^-23 * (|y2 scale2| + |shift2|) of a tie both
    neighbours are admitted (v64 .. v64_hi)."""
    p = y.double() * scale.double()
    sh = shift.double()
    v = p + sh
    mag = p.abs() + sh.abs()
    hi = None
    if aff2 is not None:
        y2, sc2, sh2 = aff2
        p2 = y2.double() * sc2.double()
        inner = p2 + sh2.double()
        d2 = 2.0 ** -23 * (p2.abs() + sh2.double().abs())
        r_lo, r_hi = bf16_rne(inner - d2), bf16_rne(inner + d2)
        mag = mag + torch.maximum(r_lo.abs(), r_hi.abs())
        v, hi = v + r_lo, v + r_hi
    elif res is not None:
        v = v + res.double()
        mag = mag + res.double().abs()
    return v, hi, 2.0 ** -22 * mag


def bn_xhat(y, mean, invstd):
    return (y.double() - mean.double()) * invstd.double()


def bn_mask_from_y(y, mean, invstd, gamma, beta):
    """MASK 2: gamma * xhat + beta > 0.  -> (m64, delta): sub, mul, and fma or mul + add: at most 4 roundings of at most
    2^-24 * (|gamma xhat| + |beta|) each."""
    t = bn_xhat(y, mean, invstd) * gamma.double()
    return t + beta.double(), 4 * U32 * (t.abs() + beta.double().abs())


def bn_bwd_apply_ref(g64, y, mean, invstd, gamma, dgamma, dbeta, rows):
    """dy = gamma invstd (g - dbeta / M - xhat dgamma / M), g the masked gradient in fp64.  -> (v64, delta).
    delta = 2^-21 * |gamma invstd| * (|g| + |dbeta / M| + |xhat dgamma / M|): eight roundings (1 / (float) rows, the
    two * invM, y - mean, * invstd, g - b1, the fma, gamma * invstd, the final product), each at most 2^-24 of a
    quantity bounded by that sum."""
    xh = bn_xhat(y, mean, invstd)
    a = gamma.double() * invstd.double()
    b1 = dbeta.double() / rows
    t2 = xh * (dgamma.double() / rows)
    v = a * (g64 - b1 - t2)
    return v, 2.0 ** -21 * a.abs() * (g64.abs() + b1.abs() + t2.abs())


def bnb_batches(rows, c):
    """bnb_batches of bn_pool.hip (the reduce aims at 1024 blocks).  -> (nbatch, rl)."""
    ncol = min(c // 8, 256)
    rl = 256 // ncol
    return max(1, min(4, -(-rows // (rl * 4 * 1024)))), rl


def bna_batches(rows, c):
    """bn_rows_batches(rows, C, 2048) of bn_pool.hip with its default knobs.  -> (nbatch, rl)."""
    ncol = min(c // 8, 256)
    rl = 256 // ncol
    return max(1, min(4, -(-rows // (rl * 4 * 2048)))), rl


def bn_bwd_sums_ref(g64, y, mean, invstd, rows, c, uncertain=None):
    """dbeta = sum g, dgamma = sum g xhat over the rows.  -> (dbeta64, bound, dgamma64, bound).
    bound = (4 nbatch + log2(rl) + 2) * 2^-24 * sum |g| (4 nbatch sequential adds per thread, the LDS tree over rl row
    lanes, the fp64 finalize's one rounding to fp32 and one of slack); 3 more for the product g * (y - mean) * invstd.
    The existing full-size test's 2e-6 is looser for every nbatch (at most 29 * 2^-24 = 1.73e-6): the derived bound is
    the one kept.  `uncertain`: elements whose mask decision is within delta of 0 -- their terms may be in or out."""
    nb, rl = bnb_batches(rows, c)
    k = 4 * nb + int(math.log2(rl)) + 2
    gx = g64 * bn_xhat(y, mean, invstd)
    bb = k * U32 * g64.abs().sum(0)
    bg = (k + 3) * U32 * gx.abs().sum(0)
    if uncertain is not None:
        bb = bb + (g64.abs() * uncertain).sum(0)
        bg = bg + (gx.abs() * uncertain).sum(0)
    return g64.sum(0), bb, gx.sum(0), bg


def colsum_ref(x, rows):
    """-> (sum64, bound): a wave adds ceil(rows / 16) terms in sequence, 16 wave sums are added in sequence."""
    x64 = x.double()
    return x64.sum(0), (-(-rows // 16) + 16) * U32 * x64.abs().sum(0)


def avgpool_ref(x, rows):
    """x [N, rows, C] -> (mean64 [N, C], bound): ceil(rows / 32) sequential adds per row lane, 32 lane sums in sequence,
    1 / (float) rows and the product."""
    x64 = x.double()
    return x64.sum(1) / rows, (-(-rows // 32) + 33) * U32 * x64.abs().sum(1) / rows


def softmax_ref(x, dtype):
    return torch.softmax(x.to(dtype), dim=1)


def softmax_bwd_ref(p, dp, scale, dtype):
    p, dp = p.to(dtype), dp.to(dtype)
    return scale * p * (dp - (dp * p).sum(1, keepdim=True))


def softmax_delta(ref64, ref32):
    """Criterion 5.  -> (delta [rows, 1], e32)."""
    e32 = float((ref32.double() - ref64).abs().max()) / (float(ref64.abs().max()) or 1.0)
    return SOFTMAX_FACTOR * e32 * ref64.abs().amax(dim=1, keepdim=True), e32


def maxpool_hw_ref(x):
    """x: NCDHW.  F.max_pool3d([1,3,3], [1,2,2], [0,1,1]) -> (y, tap bytes dh * 3 + dw as uint8, NCDHW)."""
    n, c, t, h, w = x.shape
    y, idx = torch.nn.functional.max_pool3d(x.float(), (1, 3, 3), (1, 2, 2), (0, 1, 1), return_indices=True)
    ho, wo = y.shape[3], y.shape[4]
    ih, iw = (idx % (h * w)) // w, idx % w
    oh = torch.arange(ho, device=x.device).view(1, 1, 1, ho, 1)
    ow = torch.arange(wo, device=x.device).view(1, 1, 1, 1, wo)
    tap = (ih - (2 * oh - 1)) * 3 + (iw - (2 * ow - 1))
    return y.to(x.dtype), tap.to(torch.uint8)


def maxpool_hw2_ref(x):
    """F.max_pool3d([1,2,2], [1,2,2]) -> (y, position byte (h & 1) * 2 + (w & 1))."""
    n, c, t, h, w = x.shape
    y, idx = torch.nn.functional.max_pool3d(x.float(), (1, 2, 2), (1, 2, 2), return_indices=True)
    ih, iw = (idx % (h * w)) // w, idx % w
    return y.to(x.dtype), ((ih & 1) * 2 + (iw & 1)).to(torch.uint8)


def maxpool_t_ref(x, kt):
    n, c, t, h, w = x.shape
    y, idx = torch.nn.functional.max_pool3d(x.float(), (kt, 1, 1), (kt, 1, 1), return_indices=True)
    return y.to(x.dtype), ((idx // (h * w)) % kt).to(torch.uint8)


def first_max_tap(x, y):
    """x [NT, H, W, C], y [NT, Ho, Wo, C] (3x3 s2 p1 pooled): per output the first tap in scan order whose input equals y
    (9 where none does).  For NaN-free x and y = max this is the argmax byte the kernel must store."""
    nt, h, w, c = x.shape
    ho, wo = y.shape[1], y.shape[2]
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1), value=float("-inf"))
    first = torch.full(y.shape, 9, dtype=torch.uint8, device=x.device)
    for tap in range(8, -1, -1):
        dh, dw = divmod(tap, 3)
        v = xp[:, dh:dh + 2 * ho - 1:2, dw:dw + 2 * wo - 1:2]
        first = torch.where(v == y, torch.full_like(first, tap), first)
    return first


def maxpool_hw_bwd_delta(dy, sum_abs):
    """delta of the pool backward's fp32 sum of up to 4 bf16 gradients: 2^-23 * sum |terms| in general (three adds, the
    first onto 0 exact).  Counted closer where the non-zero |dy| all lie within 2^14 of each other (binades e_m .. e_M):
    every partial sum is then a multiple of 2^(e_m - 7) below 2^(e_M + 3), i.e. fits fp32's 24 bits, every add is exact
    and delta = 0 -- the stored value IS bf16(exact sum), ties to even.  Exact sums of two bf16 values sit on rounding
    ties far too often (a quarter of the two-term sums) for a non-zero delta to stay under the ambiguity cap."""
    a = dy.double().abs()
    nz = a[a > 0]
    if nz.numel() == 0 or math.frexp(float(nz.max()))[1] - math.frexp(float(nz.min()))[1] <= 14:
        return torch.zeros_like(sum_abs)
    return 2.0 ** -23 * sum_abs


def maxpool_hw_bwd_ref(dy, idx, h, w):
    """dy, idx [NT, Ho, Wo, C] -> (dx64 [NT, H, W, C], sum |terms|): the fp64 sum of the (<= 4) window gradients whose
    argmax byte names the element (see maxpool_hw_bwd_delta)."""
    nt, ho, wo, c = dy.shape
    dev = dy.device
    ih = (2 * torch.arange(ho, device=dev) - 1).view(1, ho, 1, 1) + (idx // 3).long()
    iw = (2 * torch.arange(wo, device=dev) - 1).view(1, 1, wo, 1) + (idx % 3).long()
    ok = (ih >= 0) & (ih < h) & (iw >= 0) & (iw < w)
    flat = ((torch.arange(nt, device=dev).view(nt, 1, 1, 1) * h + ih.clamp(0, h - 1)) * w + iw.clamp(0, w - 1)) * c \
        + torch.arange(c, device=dev).view(1, 1, 1, c)
    g = torch.where(ok, dy.double(), torch.zeros((), dtype=torch.float64, device=dev)).reshape(-1)
    dx = torch.zeros(nt * h * w * c, dtype=torch.float64, device=dev).index_add_(0, flat.reshape(-1), g)
    ab = torch.zeros(nt * h * w * c, dtype=torch.float64, device=dev).index_add_(0, flat.reshape(-1), g.abs())
    return dx.view(nt, h, w, c), ab.view(nt, h, w, c)
