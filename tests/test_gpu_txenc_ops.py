"""Per-kernel parity of the fp32 encoder / head / loss / optimizer kernels (csrc/txenc_ops.hip) with plain fp64 torch
restatements, at the shapes where their dispatch turns: every instantiation of the linear forward kernels, the
KC / VEC instantiations, the in-kernel ReLU mask, the residual add and the grid-stride loop of the fused linear
backward, the attention for L <= 16 up to its largest documented head, the scalar / vector / fused / split
LayerNorm routes, the register and loop paths of the cross entropy, ties and -inf in the top-k, the second group
and second loop trip of Adam with every entry point, and the bf16 cast.

Tolerance (docs/txenc_ops_parity.md holds the measured table), the rule of tests/test_gpu_gpt2_ops.py: every case
evaluates the same restatement in fp32 torch on the CPU; its error against fp64, max |diff| / max |fp64|, is the
restatement's own fp32 noise floor `e32`.  The kernel's error, measured the same way, must be at most 16 * e32 and
never above the project's ceiling for fp32 kernels, 2e-4.  Exact paths and the bitwise claims of the source comments
are compared bit for bit.  Every figure is printed (`PARITY ...`) before it is asserted.

A compared tensor has at least 64 elements wherever the case allows it: cases with fewer outputs (n = 1 of Adam, the
3 x 5 cross entropy, dgamma at D = 1) are run on several independent draws whose results are compared as one vector.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FACTOR = 16.0
CEILING = 2e-4
NAN = float("nan")
INF = float("inf")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _errs(got, ref64, ref32):
    ref64 = ref64.detach()
    scale = float(ref64.abs().max()) or 1.0
    e32 = float((ref32.detach().double() - ref64).abs().max()) / scale
    err = float((got.detach().cpu().double() - ref64).abs().max()) / scale
    return e32, err


def _check(name, got, ref64, ref32):
    """kernel error <= min(16 * e32, 2e-4), both relative to max |fp64 reference|."""
    assert got.shape == ref64.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    e32, err = _errs(got, ref64, ref32)
    print(f"PARITY {name} e32={e32:.3e} err={err:.3e}")
    assert err <= min(FACTOR * e32, CEILING), f"{name}: kernel error {err:.3e} vs fp32 floor {e32:.3e}"


class _Calls:
    """Records the C-ABI entry points a wrapper goes through (the route taken is part of what a case is for)."""

    def __init__(self, monkeypatch, ops):
        self.names = []
        orig = ops._lib.call

        def call(name, *args):
            self.names.append(name)
            return orig(name, *args)

        monkeypatch.setattr(ops._lib, "call", call)


# ---------------------------------------------------------------------------------------------
# 1. linear forward
# ---------------------------------------------------------------------------------------------
GELU_K, GELU_C = math.sqrt(2.0 / math.pi), 0.044715


def _gelu_new(x):  # oracle/gpt2_ref.py
    return 0.5 * x * (1.0 + torch.tanh(GELU_K * (x + GELU_C * x * x * x)))


def _linear_inputs(m, n, k, seed=0):
    g = _gen(1000003 * m + 1009 * n + k + seed)
    x = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) / k ** 0.5
    b = torch.randn(n, generator=g)
    return g, x, w, b


LINEAR_FWD_CASES = [
    # linear_fullx_kernel<8, 4>: K <= 1024
    (1, 64, 4), (8, 65, 1024),
    # <8, 8>: the second register chunk is one float4 column; K = 2048
    (8, 65, 1028), (7, 64, 2048),
    # <8, 16>: 2048 < K <= 4096, two staged chunks of x
    (8, 64, 2052), (5, 66, 4096),
    # <16, 4> / <16, 8>
    (9, 64, 1024), (16, 67, 1028), (16, 64, 2048),
    # linear_fwd_kernel<8>: M <= 8 with K > 4096 (second trip of the kg loop)
    (8, 64, 4100),
    # linear_fwd_kernel<16>: vector loads (M 9..16, K > 2048), scalar loads (K % 4 != 0)
    (12, 65, 2052), (13, 64, 1027),
    # linear_fwd_kernel<32>, <48>
    (17, 64, 1025), (48, 9, 259),
    # linear_fwd_kernel<64>: one slab; two row slabs and the second kg trip
    (64, 5, 1030), (130, 7, 1026),
    # linear_rows16_kernel: M > 16, K % 4 == 0; one, two and four row blocks, one and two K chunks
    (17, 64, 4), (33, 70, 1028), (64, 16, 2048),
]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("m,n,k", LINEAR_FWD_CASES, ids=[f"{m}x{n}x{k}" for m, n, k in LINEAR_FWD_CASES])
def test_linear_fwd(m, n, k, relu, dev):
    """Every kernel `linear_small_m` can choose (the comments of LINEAR_FWD_CASES name the branch of each case)."""
    from vidsitu_amd import ops

    _, x, w, b = _linear_inputs(m, n, k)

    def ref(dt):
        y = x.to(dt) @ w.to(dt).t() + b.to(dt)
        return torch.relu(y) if relu else y

    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    y = ops.linear_fwd(xd, wd, bd, bool(relu))
    _check(f"linear_fwd {m}x{n}x{k} relu{relu}", y, ref(torch.float64), ref(torch.float32))
    assert _same_bits(y, ops.linear_fwd(xd, wd, bd, bool(relu))), "two runs differ"
    if relu:
        assert float(y.min()) >= 0.0


GEMM_NT_CASES = [(8, 64, 1024), (16, 65, 2048), (13, 64, 1027), (50, 24, 1028), (40, 10, 1027)]


@pytest.mark.parametrize("m,n,k", GEMM_NT_CASES, ids=[f"{m}x{n}x{k}" for m, n, k in GEMM_NT_CASES])
def test_gemm_nt_gelu_new_and_residual_on_declined_rows(m, n, k, dev):
    """act = 2 (gelu_new) and the residual through the kernels behind `vs_gemm_nt_f32` when the skinny MFMA kernel
    declines: M <= 16 (fullx<8,4>, fullx<16,8>, linear_fwd_kernel<16>), K % 128 != 0 (rows16, linear_fwd_kernel<48>)."""
    from vidsitu_amd import ops

    g, x, w, b = _linear_inputs(m, n, k, seed=7)
    res = torch.randn(m, n, generator=g)

    def ref(dt):
        return _gelu_new(x.to(dt) @ w.to(dt).t() + b.to(dt)) + res.to(dt)

    args = (x.to(dev), w.to(dev), b.to(dev), res.to(dev), ops.ACT_GELU_NEW)
    y = ops.gemm_nt(*args)
    _check(f"gemm_nt gelu_new+res {m}x{n}x{k}", y, ref(torch.float64), ref(torch.float32))
    out = torch.full((m, n), NAN, device=dev)
    assert _same_bits(y, ops.gemm_nt(*args, out=out)), "two runs differ"


# ---------------------------------------------------------------------------------------------
# 2. linear backward, transpose
# ---------------------------------------------------------------------------------------------
def _linear_bwd_inputs(m, n, k):
    g, x, w, _ = _linear_inputs(m, n, k, seed=3)
    dy = torch.randn(m, n, generator=g)
    relu_y = torch.relu(torch.randn(m, n, generator=g))  # a real ReLU output: about half of it exact zeros
    relu_y[0, 0] = -0.0  # -0 is not > 0
    dx_res = torch.randn(m, k, generator=g)
    return x, w, dy, relu_y, dx_res


def _linear_bwd_ref(dt, x, w, dy, relu_y, dx_res):
    dy_eff = dy.to(dt)
    if relu_y is not None:
        dy_eff = dy_eff * (relu_y > 0).to(dt)
    dx = dy_eff @ w.to(dt)
    if dx_res is not None:
        dx = dx + dx_res.to(dt)
    return dx, dy_eff.t() @ x.to(dt), dy_eff.sum(0)


def _linear_bwd_three_launches(ops, dyd, xd, wd, relu_d, res_d, has_bias, dev):
    """relu_bwd, vs_linear_bwd_data and vs_linear_bwd_weight, called the way `ops.linear_bwd`'s fallback calls them."""
    m, n = dyd.shape
    k = xd.shape[1]
    if relu_d is not None:
        dyd = ops.relu_bwd(dyd, relu_d)
    wt = ops.transpose_f32(wd)
    dx = torch.full((m, k), NAN, device=dev)
    ops._lib.call("vs_linear_bwd_data", ops._ptr(dyd), ops._ptr(wt), ops._ptr(dx), m, n, k, ops._stream())
    dw = torch.full((n, k), NAN, device=dev)
    db = torch.full((n,), NAN, device=dev) if has_bias else None
    ops._lib.call("vs_linear_bwd_weight", ops._ptr(dyd), ops._ptr(xd), ops._ptr(dw), ops._ptr(db), m, n, k,
                  ops._stream())
    if res_d is not None:
        dx = dx + res_d
    return dx, dw, db


LINEAR_BWD_FUSED_CASES = [
    (5, 64, 7),        # VEC = false (K % 4 != 0), KC 4
    (8, 1024, 12),     # KC 4 at its last N
    (8, 1028, 12),     # KC 8 at its first N
    (3, 2048, 10),     # KC 8 at its last N, VEC = false
    (8, 2052, 2052),   # KC 16 at its first N, and the weight half's grid-stride loop (2052 * 513 > 4096 * 256)
    (1, 4096, 8),      # KC 16 at its last N
]


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("with_relu", [False, True], ids=["norelu", "relu"])
@pytest.mark.parametrize("m,n,k", LINEAR_BWD_FUSED_CASES, ids=[f"{m}x{n}x{k}" for m, n, k in LINEAR_BWD_FUSED_CASES])
def test_linear_bwd_fused(m, n, k, with_relu, with_res, dev, monkeypatch):
    """`vs_linear_bwd_fused_res` through `ops.linear_bwd` (M <= 8, N % 4 == 0): every KC, both VEC, the ReLU mask and
    the residual given to the kernel itself, against fp64 and bit for bit against the three launches it replaces
    (its kernel comment claims that).  dx of the narrow cases has fewer than 64 elements; each is a sum over N >= 64."""
    from vidsitu_amd import ops

    x, w, dy, relu_y, dx_res = _linear_bwd_inputs(m, n, k)
    relu_y = relu_y if with_relu else None
    dx_res = dx_res if with_res else None
    xd, wd, dyd = x.to(dev), w.to(dev), dy.to(dev)
    relu_d = None if relu_y is None else relu_y.to(dev)
    res_d = None if dx_res is None else dx_res.to(dev)
    calls = _Calls(monkeypatch, ops)
    dx, dw, db = ops.linear_bwd(dyd, xd, wd, relu_y=relu_d, dx_res=res_d)
    assert calls.names == ["vs_transpose_f32", "vs_linear_bwd_fused_res"], calls.names
    name = f"linear_bwd_fused {m}x{n}x{k}{' relu' if with_relu else ''}{' res' if with_res else ''}"
    r64 = _linear_bwd_ref(torch.float64, x, w, dy, relu_y, dx_res)
    r32 = _linear_bwd_ref(torch.float32, x, w, dy, relu_y, dx_res)
    for part, got, a, b in zip(("dx", "dw", "db"), (dx, dw, db), r64, r32):
        _check(f"{name} {part}", got, a, b)
    dx3, dw3, db3 = _linear_bwd_three_launches(ops, dyd, xd, wd, relu_d, res_d, True, dev)
    assert _same_bits(dx, dx3) and _same_bits(dw, dw3) and _same_bits(db, db3), "fused launch != the three launches"


def test_linear_bwd_fused_without_bias(dev, monkeypatch):
    """has_bias = False: db is a null pointer inside the weight half."""
    from vidsitu_amd import ops

    m, n, k = 5, 64, 7
    x, w, dy, relu_y, dx_res = _linear_bwd_inputs(m, n, k)
    xd, wd, dyd, relu_d, res_d = (t.to(dev) for t in (x, w, dy, relu_y, dx_res))
    calls = _Calls(monkeypatch, ops)
    dx, dw, db = ops.linear_bwd(dyd, xd, wd, has_bias=False, relu_y=relu_d, dx_res=res_d)
    assert db is None and calls.names[-1] == "vs_linear_bwd_fused_res"
    r64 = _linear_bwd_ref(torch.float64, x, w, dy, relu_y, dx_res)
    r32 = _linear_bwd_ref(torch.float32, x, w, dy, relu_y, dx_res)
    _check(f"linear_bwd_fused {m}x{n}x{k} relu res nobias dx", dx, r64[0], r32[0])
    _check(f"linear_bwd_fused {m}x{n}x{k} relu res nobias dw", dw, r64[1], r32[1])
    dx3, dw3, _ = _linear_bwd_three_launches(ops, dyd, xd, wd, relu_d, res_d, False, dev)
    assert _same_bits(dx, dx3) and _same_bits(dw, dw3)


LINEAR_BWD_UNFUSED_CASES = [
    (9, 1024, 12),     # M > 8: data gradient on fullx<16, 4>
    (8, 1027, 12),     # N % 4 != 0: data gradient on linear_fwd_kernel<8>
    (16, 64, 130),     # the weight kernel's row batches of 8: exactly two
    (17, 64, 130),     # ... and a third with one row; data gradient on rows16
    (9, 2052, 2052),   # the weight kernel's grid-stride loop; data gradient on linear_fwd_kernel<16>
]


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "relu_res"])
@pytest.mark.parametrize("m,n,k", LINEAR_BWD_UNFUSED_CASES,
                         ids=[f"{m}x{n}x{k}" for m, n, k in LINEAR_BWD_UNFUSED_CASES])
def test_linear_bwd_unfused(m, n, k, extras, dev, monkeypatch):
    """`vs_linear_bwd_data` + `vs_linear_bwd_weight` (and `vs_relu_bwd` in front when a ReLU output is given)."""
    from vidsitu_amd import ops

    x, w, dy, relu_y, dx_res = _linear_bwd_inputs(m, n, k)
    relu_y, dx_res = (relu_y, dx_res) if extras else (None, None)
    calls = _Calls(monkeypatch, ops)
    dx, dw, db = ops.linear_bwd(dy.to(dev), x.to(dev), w.to(dev), relu_y=None if relu_y is None else relu_y.to(dev),
                                dx_res=None if dx_res is None else dx_res.to(dev))
    want = ["vs_transpose_f32", "vs_linear_bwd_data", "vs_linear_bwd_weight"]
    assert calls.names == (["vs_relu_bwd"] if extras else []) + want, calls.names
    name = f"linear_bwd_unfused {m}x{n}x{k}{' relu res' if extras else ''}"
    r64 = _linear_bwd_ref(torch.float64, x, w, dy, relu_y, dx_res)
    r32 = _linear_bwd_ref(torch.float32, x, w, dy, relu_y, dx_res)
    for part, got, a, b in zip(("dx", "dw", "db"), (dx, dw, db), r64, r32):
        _check(f"{name} {part}", got, a, b)


@pytest.mark.parametrize("r,c", [(64, 1), (33, 31), (1027, 12)])
def test_transpose_f32(r, c, dev):
    """Bit for bit `.t().contiguous()`; the destination sits inside a NaN-filled buffer and nothing around it is
    written (partial 32 x 32 tiles on both sides)."""
    from vidsitu_amd import ops

    x = torch.randn(r, c, generator=_gen(r * 100 + c))
    xd = x.to(dev)
    pad = 64
    buf = torch.full((r * c + 2 * pad,), NAN, device=dev)
    dst = buf[pad:pad + r * c]
    ops._lib.call("vs_transpose_f32", ops._ptr(xd), ops._ptr(dst), r, c, ops._stream())
    torch.cuda.synchronize()
    assert _same_bits(dst.view(c, r), x.t().contiguous())
    assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + r * c:]).all()), "wrote outside [C, R]"
    assert _same_bits(ops.transpose_f32(xd), x.t().contiguous())


# ---------------------------------------------------------------------------------------------
# 3. attention for L <= 16
# ---------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, mask, h, scale):
    """utils/transformer_code.py Attention per head: softmax(q k^T / scale) (* dropout mask) v -> (o, probs)."""
    b, l, d = q.shape
    dh = d // h
    qh, kh, vh = (t.view(b, l, h, dh).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) / scale, -1)
    pd = p if mask is None else p * mask.to(p.dtype)
    return (pd @ vh).transpose(1, 2).reshape(b, l, d), p


def _attn_case(b, l, h, dh, with_mask, qscale):
    g = _gen(10007 * b + 101 * l + 13 * h + dh + int(with_mask))
    d = h * dh
    qkv = torch.randn(b * l, 3 * d, generator=g)
    qkv[:, :d] *= qscale
    do = torch.randn(b, l, d, generator=g)
    mask = (torch.rand(b, h, l, l, generator=g) >= 0.25).float() / 0.75 if with_mask else None
    out = {}
    for dt in (torch.float64, torch.float32):
        x = qkv.to(dt).requires_grad_(True)
        q, k, v = (x[:, i * d:(i + 1) * d].reshape(b, l, d) for i in range(3))
        o, p = _attn_ref(q, k, v, mask, h, float(d) ** 0.5)
        gx, = torch.autograd.grad(o, x, do.to(dt))
        out[dt] = (o.detach(), p.detach(), gx)
    return qkv, do, mask, out[torch.float64], out[torch.float32]


ATTN_CASES = [  # B, L, H, dh, scale of q
    (2, 1, 2, 64, 1.0),     # one key: every probability is exactly 1
    (2, 2, 3, 8, 1.0),
    (1, 15, 2, 40, 1.0),    # L * L = 225 < 256 threads, dh no power of two
    (1, 16, 2, 16, 1.0),    # L * L = 256: one full trip of the 256-thread loops
    (2, 5, 8, 128, 1.0),    # the encoder's own shape
    (1, 16, 1, 256, 1.0),   # backward needs 68 608 B of LDS (> 64 KiB)
    (1, 16, 1, 512, 1.0),   # the largest documented head: 99 328 B forward, 134 144 B backward
    (1, 15, 2, 40, 30.0),   # scores of +-30 and more: the max subtraction
]


@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "dropmask"])
@pytest.mark.parametrize("b,l,h,dh,qscale", ATTN_CASES,
                         ids=[f"B{c[0]}_L{c[1]}_H{c[2]}_dh{c[3]}" + ("_q30" if c[4] != 1 else "") for c in ATTN_CASES])
def test_attn_small(b, l, h, dh, qscale, with_mask, dev):
    """`vs_attn_small_fwd` / `_bwd` over their documented range (L <= 16, dh <= 512), separate q / k / v tensors and the
    fused-qkv layout (row pitch 3 D), forward output, saved probabilities and the three gradients.  dq | dk | dv of the
    fused layout start as NaN: every element has an owner.  Both layouts run the same code: equal bits.
    The wrappers ask for up to 134 144 B of dynamic LDS (L = 16, dh = 512, backward) without raising the kernels'
    limit first; on gfx950 the runtime grants it (160 KiB per workgroup), so the documented range runs as it is."""
    from vidsitu_amd import ops

    qkv, do, mask, r64, r32 = _attn_case(b, l, h, dh, with_mask, qscale)
    d = h * dh
    scale = float(d) ** 0.5
    name = f"attn_small B{b} L{l} H{h} dh{dh}{' q*30' if qscale != 1 else ''}{' dropmask' if with_mask else ''}"
    qkv_d, do_d = qkv.to(dev), do.to(dev)
    mask_d = None if mask is None else mask.to(dev)
    q, k, v = (qkv_d[:, i * d:(i + 1) * d].reshape(b, l, d).contiguous() for i in range(3))
    o, probs = ops.attn_small_fwd(q, k, v, h, scale, mask_d)
    _check(f"{name} o", o, r64[0], r32[0])
    _check(f"{name} probs", probs, r64[1], r32[1])
    o_f, probs_f = ops.attn_small_fwd_fused(qkv_d, b, l, h, scale, mask_d)
    assert _same_bits(o, o_f) and _same_bits(probs, probs_f), "fused-qkv forward != separate q / k / v"
    dq, dk, dv = ops.attn_small_bwd(q, k, v, probs, do_d, h, scale, mask_d)
    dqkv = torch.full_like(qkv_d, NAN)
    ops._lib.call("vs_attn_small_bwd", ops._ptr(qkv_d), ops._ptr(qkv_d[:, d:]), ops._ptr(qkv_d[:, 2 * d:]),
                  ops._ptr(probs), ops._ptr(do_d), ops._ptr(dqkv), ops._ptr(dqkv[:, d:]), ops._ptr(dqkv[:, 2 * d:]),
                  ops._ptr(mask_d), b, l, h, dh, 3 * d, scale, ops._stream())
    assert bool(torch.isfinite(dqkv).all()), "an element of dqkv was not written"
    for i, (part, sep) in enumerate((("dq", dq), ("dk", dk), ("dv", dv))):
        sl = slice(i * d, (i + 1) * d)
        _check(f"{name} {part}", dqkv[:, sl], r64[2][:, sl], r32[2][:, sl])
        assert _same_bits(sep.reshape(b * l, d), dqkv[:, sl]), f"fused-qkv {part} != separate q / k / v"
    assert _same_bits(dqkv, ops.attn_small_bwd_fused(qkv_d, probs, do_d, b, l, h, scale, mask_d)), "two runs differ"


def test_attn_small_refuses_what_it_documents_as_out_of_range(dev):
    """L = 17 and dh = 513 are bad-argument errors that launch nothing."""
    from vidsitu_amd import ops

    for b, l, h, dh in ((1, 17, 1, 8), (1, 2, 1, 513)):
        q = torch.zeros(b, l, h * dh, device=dev)
        with pytest.raises(ops._lib.VsError, match="vs_status"):
            ops.attn_small_fwd(q, q, q, h, 1.0)


# ---------------------------------------------------------------------------------------------
# 4. LayerNorm(x + r * rmask)
# ---------------------------------------------------------------------------------------------
LN_EPS = 1e-5
LN_MODES = ("x", "x+r", "x+r*mask")
LN_CONST_DY = 2.0 ** -8  # the constant row's rstd is eps^-1/2 = 316: its dy is scaled down so that its dx is of order 1


def _ln_special_rows(rows):
    """(constant row, row with mean 1e3); None where the case has too few rows to hold them beside a normal one."""
    return (1, rows - 1) if rows >= 3 else (None, None)


def _ln_inputs(rows, d, mode, seed=0):
    g = _gen(100003 * rows + 17 * d + LN_MODES.index(mode) + seed)
    x = torch.randn(rows, d, generator=g)
    r = torch.randn(rows, d, generator=g) if mode != "x" else None
    rmask = (torch.rand(rows, d, generator=g) >= 0.5).float() * 2.0 if mode == "x+r*mask" else None  # dropout 0.5
    gamma = torch.rand(d, generator=g) + 0.5
    beta = torch.randn(d, generator=g)
    const, big = _ln_special_rows(rows)
    if const is not None:
        # x + r * rmask = 0.75 in every column: sums of multiples of 0.25 are exact in any order, the mean is exactly
        # 0.75 and the variance exactly 0 in fp32 as in fp64
        if mode == "x":
            x[const] = 0.75
        elif mode == "x+r":
            x[const], r[const] = 0.5, 0.25
        else:
            x[const], r[const] = 0.75, 0.0
        # Mean 1e3, unit spread, every entry of x, r and x + r * rmask on a grid of 1/8 and below 1012: the row's sum
        # is below 2^24 / 8 for D <= 2048, hence exact in fp32 in ANY order, and the mean is that sum divided by D in
        # the kernel as in fp32 torch.  Otherwise the one rounding of one sum would be this row's whole fp32 floor
        # (6e-5 of its spread per ulp), and whether a kernel passed would be the luck of that rounding; what the row
        # is for -- the centred second pass instead of E[v^2] - mean^2 -- does not depend on it.
        x[big] = 1e3 + (x[big] * 8).round().clamp(-24, 24) / 8
        if r is not None:
            r[big] = (r[big] * 8).round().clamp(-16, 16) / 8
    return x, r, rmask, gamma, beta, g


def _ln_ref(dt, x, r, rmask, gamma, beta, dys):
    """-> y, mean, rstd and, per dy, (dx, dr, dgamma, dbeta), by autograd through the plain formula."""
    xx = x.to(dt).requires_grad_(True)
    rr = None if r is None else r.to(dt).requires_grad_(True)
    gg, bb = gamma.to(dt).requires_grad_(True), beta.to(dt).requires_grad_(True)
    v = xx if rr is None else xx + (rr if rmask is None else rr * rmask.to(dt))
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    y = (v - mean) * rstd * gg + bb
    grads = []
    for dy in dys:
        ins = [xx, gg, bb] + ([rr] if rr is not None else [])
        gs = torch.autograd.grad(y, ins, dy.to(dt), retain_graph=True)
        grads.append((gs[0], gs[3] if rr is not None else gs[0], gs[1], gs[2]))
    return y.detach(), mean.detach().reshape(-1), rstd.detach().reshape(-1), grads


def _check_rows(name, got, ref64, ref32, big):
    """The row with mean 1e3 has an fp32 floor of its own (one ulp of its entries is 6e-5 of its spread): where both
    parts have 64 elements it is compared apart from the other rows, so that it does not set their bound."""
    rows, d = ref64.shape
    if big is None or d < 64 or (rows - 1) * d < 64:
        return _check(name, got, ref64, ref32)
    rest = torch.arange(rows) != big
    _check(name, got[rest.to(got.device)], ref64[rest], ref32[rest])
    _check(f"{name} [mean 1e3 row]", got[big], ref64[big], ref32[big])


def _ln_run(ops, dev, name, rows, d, mode, offset=0):
    """One shape and mode, forward and backward.  The backward gets the forward kernel's own mean / rstd, as in the
    model.  mean / rstd are held to the rule where there are 64 rows of them; below that they are covered through y
    and dx.  dgamma / dbeta of D < 64 are compared over ceil(64 / D) draws of dy as one vector."""
    x, r, rmask, gamma, beta, g = _ln_inputs(rows, d, mode)
    const, big = _ln_special_rows(rows)
    ndraw = max(1, -(-64 // d))
    dys = [torch.randn(rows, d, generator=g) for _ in range(ndraw)]
    if const is not None:
        for dy in dys:
            dy[const] *= LN_CONST_DY
    y64, mean64, rstd64, g64 = _ln_ref(torch.float64, x, r, rmask, gamma, beta, dys)
    y32, mean32, rstd32, g32 = _ln_ref(torch.float32, x, r, rmask, gamma, beta, dys)

    def put(t):
        """On the device; with `offset` as a view `offset` floats into a larger buffer (not 16-byte aligned)."""
        if t is None:
            return None
        if not offset:
            return t.to(dev)
        buf = torch.zeros(t.numel() + 8, device=dev)
        view = buf[offset:offset + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
        return view

    xd, rd, md, gd, bd = put(x), put(r), put(rmask), put(gamma), put(beta)
    y, mean, rstd = ops.add_layernorm_fwd(xd, rd, gd, bd, LN_EPS, md)
    _check_rows(f"{name} y", y, y64, y32, big)
    if rows >= 64:
        _check(f"{name} mean", mean, mean64, mean32)
        _check(f"{name} rstd", rstd, rstd64, rstd32)
    if const is not None:
        assert _same_bits(y[const], beta), "variance 0: the row must be beta exactly"
    dgs, dbs = [], []
    for i, dy in enumerate(dys):
        dx, dr, dg, db = ops.add_layernorm_bwd(put(dy), xd, rd, gd, mean, rstd, md)
        if i == 0:
            _check_rows(f"{name} dx", dx, g64[0][0], g32[0][0], big)
            if mode == "x+r*mask":
                _check_rows(f"{name} dr", dr, g64[0][1], g32[0][1], big)
                assert _same_bits(dr, dx * md), "dr != dx * rmask"
            else:
                assert dr is dx
        dgs.append(dg)
        dbs.append(db)
    _check(f"{name} dgamma", torch.cat(dgs), torch.cat([t[2] for t in g64]), torch.cat([t[2] for t in g32]))
    _check(f"{name} dbeta", torch.cat(dbs), torch.cat([t[3] for t in g64]), torch.cat([t[3] for t in g32]))
    return y, mean, rstd


def _ln_rows_for(d):
    return max(5, -(-64 // d))  # five rows, or as many as 64 compared elements of y need (D = 1, 4)


LN_D_VECTOR = [4, 60, 64, 68, 252, 256, 260, 1024, 1028, 2044, 2048]
LN_D_SCALAR = [1, 63, 65, 101, 1023, 2047]
LN_ROWS = [1, 3, 4, 5, 16, 17, 63, 64, 65, 130]


@pytest.mark.parametrize("d", LN_D_VECTOR + LN_D_SCALAR)
def test_add_layernorm_every_width(d, dev):
    """Vector kernels (D % 4 == 0): 63 / 64 / 65 float4 columns per row (252 / 256 / 260: the second register column
    of a lane), 1024 / 1028 (the last D of the fused backward and the first of the split vector route), 2044 / 2048
    (the last register column), 60 / 64 / 68 (one / one full / two 64-column blocks of the parameter pass).  Scalar
    kernels (D % 4 != 0): one column (every row has variance 0), 63 / 65 around the wave width, 1023 and 2047."""
    from vidsitu_amd import ops

    rows = _ln_rows_for(d)
    for mode in LN_MODES:
        _ln_run(ops, dev, f"add_layernorm {rows}x{d} {mode}", rows, d, mode)


@pytest.mark.parametrize("d", [64, 1028])
@pytest.mark.parametrize("rows", LN_ROWS)
def test_add_layernorm_every_row_count(rows, d, dev):
    """rows 1 / 3 / 4 / 5 (idle waves of a block, a second block), 16 / 17 (the fused backward's input-gradient blocks
    1 -> 2), 63 / 64 / 65 (last fused launch -> split route; the parameter pass's second trip, `row0 += 64`), 130
    (third trip).  D = 64 takes the fused launch up to 64 rows, D = 1028 the split vector route throughout."""
    from vidsitu_amd import ops

    for mode in LN_MODES:
        _ln_run(ops, dev, f"add_layernorm {rows}x{d} {mode}", rows, d, mode)


def test_add_layernorm_misaligned_view_takes_scalar_kernels(dev):
    """D % 4 == 0 on views one float into larger buffers: the dispatcher's 16-byte test must route them to the scalar
    kernels (`put` asserts the misalignment).  The result holds the rule, and it is the scalar kernels' summation
    order, not the vector kernels': the bits differ from the aligned run."""
    from vidsitu_amd import ops

    rows, d = 5, 1024
    outs = [_ln_run(ops, dev, f"add_layernorm {rows}x{d} x+r*mask {tag}", rows, d, "x+r*mask", offset=off)
            for tag, off in (("aligned", 0), ("misaligned", 1))]
    assert not all(_same_bits(a, b) for a, b in zip(*outs)), "same bits as the vector kernel: which kernel ran?"


@pytest.mark.parametrize("d", [16, 2048])
@pytest.mark.parametrize("rows", [16, 17])
def test_layernorm_fwd_packed_is_the_row_major_result(rows, d, dev):
    """`vs_layernorm_fwd_packed` (fragment-major output) against the row-major kernel, bit for bit."""
    from vidsitu_amd import ops

    x, _, _, gamma, beta, _ = _ln_inputs(rows, d, "x")
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    y, _, _ = ops.add_layernorm_fwd(xd, None, gd, bd, LN_EPS)
    packed = ops.layernorm_fwd_packed(xd, gd, bd, LN_EPS)
    assert _same_bits(ops.unpack_rows_f32(packed, rows, d), y)


# ---------------------------------------------------------------------------------------------
# 5. cross entropy, top-k
# ---------------------------------------------------------------------------------------------
N_LABEL_SETS = 8


def _xent_labels(g, rows, v, s):
    labels = torch.randint(0, v, (rows,), generator=g)
    if rows >= 2:
        labels[0], labels[-1] = 0, v - 1
    else:
        labels[0] = (0, v - 1)[s % 2]
    return labels


def _xent_ref(dt, logits, labels):
    x = logits.to(dt).requires_grad_(True)
    loss = F.cross_entropy(x, labels)
    g, = torch.autograd.grad(loss, x)
    return loss.detach().reshape(1), g


def _xent_run(ops, dev, name, rows, v, spread=False):
    """The loss as a vector over eight label sets (docs/gpt2_ops_parity.md: one scalar's fp32 floor can be almost 0 by
    luck), dlogits of the first set; small cases repeat over independent logits until 64 elements are compared."""
    g = _gen(100003 * rows + v + int(spread))
    ndraw = max(1, -(-64 // (rows * v)))
    got_l, l64, l32, got_g, g64, g32 = [], [], [], [], [], []
    for _ in range(ndraw):
        logits = torch.randn(rows, v, generator=g) * 3.0
        sets = [_xent_labels(g, rows, v, s) for s in range(N_LABEL_SETS)]
        if spread:  # +80 and -80 in one row (exp(80) overflows fp32 without the max subtraction); the label on the -80
            logits[0, 1], logits[0, v // 2], logits[rows - 1, v - 1] = 80.0, -80.0, 80.0
            for lb in sets:
                lb[0] = v // 2
        ld = logits.to(dev)
        for s, labels in enumerate(sets):
            lbd = labels.to(dev)
            loss, dl = ops.softmax_xent(ld, lbd, want_grad=(s == 0))
            got_l.append(loss.reshape(1).cpu())
            a, ga = _xent_ref(torch.float64, logits, labels)
            b, gb = _xent_ref(torch.float32, logits, labels)
            l64.append(a)
            l32.append(b)
            if s == 0:
                got_g.append(dl.cpu().reshape(-1))
                g64.append(ga.reshape(-1))
                g32.append(gb.reshape(-1))
                loss_nograd, none = ops.softmax_xent(ld, lbd, want_grad=False)
                assert none is None and _same_bits(loss.reshape(1), loss_nograd.reshape(1)), "loss depends on want_grad"
    _check(f"softmax_xent {name} loss", torch.cat(got_l), torch.cat(l64), torch.cat(l32))
    _check(f"softmax_xent {name} dlogits", torch.cat(got_g), torch.cat(g64), torch.cat(g32))


XENT_CASES = [(1, 64), (3, 5), (4, 63), (5, 65), (9, 2047), (9, 2048), (9, 2049), (6, 5000)]


@pytest.mark.parametrize("rows,v", XENT_CASES, ids=[f"{r}x{v}" for r, v in XENT_CASES])
def test_softmax_xent(rows, v, dev):
    """Register path (V <= 2048) and loop path: rows < 4 (idle waves add 0 to the loss), V < 64 (idle lanes), 63 / 65,
    the 2047 / 2048 / 2049 edge between the paths, 5000 (the loop path well inside); rows 5, 6, 9: a wave with two and
    three rows.  Labels include 0 and V - 1."""
    from vidsitu_amd import ops

    _xent_run(ops, dev, f"{rows}x{v}", rows, v)


@pytest.mark.parametrize("rows,v", [(5, 65), (9, 2049)], ids=["5x65", "9x2049"])
def test_softmax_xent_large_logits(rows, v, dev):
    from vidsitu_amd import ops

    _xent_run(ops, dev, f"{rows}x{v} +-80", rows, v, spread=True)


def _topk_check(ops, dev, name, logits, k):
    rows, v = logits.shape
    order = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :k]
    probs, idx = ops.softmax_topk(logits.to(dev), k)
    assert idx.dtype == torch.int64 and torch.equal(idx.cpu(), order), f"{name}: indices"
    p64 = torch.softmax(logits.double(), -1).gather(1, order)
    p32 = torch.softmax(logits, -1).gather(1, order)
    _check(f"softmax_topk {name}", probs, p64, p32)
    return probs, idx


TOPK_CASES = [(22, 3, 3), (13, 64, 5), (13, 65, 5), (64, 100, 1), (13, 1564, 5)]


@pytest.mark.parametrize("rows,v,k", TOPK_CASES, ids=[f"{r}x{v}_k{k}" for r, v, k in TOPK_CASES])
def test_softmax_topk(rows, v, k, dev):
    """Indices exact against a stable descending sort of the logits; V = k = 3, V = 64 / 65, k = 1, the verb head."""
    from vidsitu_amd import ops

    logits = torch.randn(rows, v, generator=_gen(rows * 10007 + v)) * 2.0
    _topk_check(ops, dev, f"{rows}x{v} k{k}", logits, k)


def test_softmax_topk_ties_and_minus_inf(dev):
    """Equal values at j and j + 64 (the same lane meets both) and at j, j + 1 (neighbouring lanes), an all-equal row,
    more ties than k, and rows with -inf entries that k reaches into (probability exactly 0, lowest index first)."""
    from vidsitu_amd import ops

    v, k = 200, 5
    logits = torch.randn(16, v, generator=_gen(5)) * 2.0
    logits[0, 70], logits[0, 6] = 9.0, 9.0                      # j and j + 64
    logits[1, 133], logits[1, 5], logits[1, 69] = 9.0, 9.0, 9.0  # j, j + 64, j + 128
    logits[2, 10], logits[2, 11] = 9.0, 9.0
    logits[3] = 1.25                                             # all equal
    logits[4, 20:60] = 7.0                                       # forty ties for five places
    logits[5, 100:] = -INF
    logits[6] = -INF
    logits[6, [190, 3, 64]] = torch.tensor([0.5, 0.5, -1.0])     # three finite values: places 4 and 5 are -inf
    logits[7, :] = -INF
    logits[7, 199] = 0.0                                         # one finite value
    probs, idx = _topk_check(ops, dev, f"16x{v} k{k} ties/-inf", logits, k)
    assert idx[0, :2].tolist() == [6, 70] and idx[1, :3].tolist() == [5, 69, 133] and idx[2, :2].tolist() == [10, 11]
    assert idx[3].tolist() == [0, 1, 2, 3, 4] and idx[4].tolist() == [20, 21, 22, 23, 24]
    assert idx[6].tolist() == [3, 190, 64, 0, 1] and probs[6, 3:].tolist() == [0.0, 0.0]
    assert idx[7].tolist() == [199, 0, 1, 2, 3] and probs[7].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]


# ---------------------------------------------------------------------------------------------
# 6. Adam, bf16 cast
# ---------------------------------------------------------------------------------------------
def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


# lr, betas (the reference trainer's 0.9, 0.99) and eps.  The C ABI takes them as floats, so like every tensor input of
# these fp32 kernels they enter the restatement as the fp32 values the kernel receives, promoted: 0.99f is
# 0.9900000095..., and 1 - 0.99f is 9.5e-7 (relative) below 0.01 -- see test_adam_betas_arrive_as_floats.
ADAM_DOUBLES = (1e-3, 0.9, 0.99, 1e-8)
LR, B1, B2, EPS = (_f32(c) for c in ADAM_DOUBLES)


def _adam_ref(dt, p, g, m, v, step, gs, consts=(LR, B1, B2, EPS)):
    """torch.optim.Adam: the bias corrections are formed in Python doubles."""
    lr, b1, b2, eps = consts
    p, g, m, v = p.to(dt), g.to(dt) * gs, m.to(dt), v.to(dt)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def _adam_inputs(n, step, p0zero, seed=0):
    g = _gen(n * 31 + step + seed)
    p = torch.zeros(n) if p0zero else torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g)
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m, v = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
    zero = []
    if n >= 1023:
        # exactly-zero gradients on zero moments: the update is exactly 0.  Stretches at the front, across the boundary
        # between the first and the second float4 group of the full grid (float index 4 * 4096 * 256), and the tail
        zero = [slice(16, 48), slice(n - 37, n)]
        if n > 4 * 1048576:
            zero.append(slice(4 * 1048576 - 8, 4 * 1048576 + 8))
        for sl in zero:
            gr[sl], m[sl], v[sl] = 0.0, 0.0, 0.0
    return p, gr, m, v, zero


def _view(t, dev, offset):
    """t on the device; with `offset` as a view one element into a larger buffer."""
    if not offset:
        return t.to(dev)
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=dev)
    view = buf[1:1 + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


ADAM_VARIANTS = ("step", "dev", "cast", "cast_g16", "range", "range_pb", "range_g16", "range_g16_pb")


def _adam_launch(ops, dev, variant, p, g, m, v, step, gs, offset=False):
    """One update through `variant`, the step counter preset so that the step taken is `step` -> p, m, v, p_bf16."""
    pd, md, vd = (_view(t.clone(), dev, offset) for t in (p, m, v))
    g16 = variant.endswith("g16") or variant.endswith("g16_pb")
    gd = _view(g.to(torch.bfloat16) if g16 else g, dev, offset)
    pb = None
    if variant in ("cast", "cast_g16", "range_pb", "range_g16_pb"):
        pb = _view(torch.zeros(p.numel(), dtype=torch.bfloat16), dev, offset)
    cnt = torch.tensor([step - 1], dtype=torch.int32, device=dev)
    args = (LR, B1, B2, EPS)
    if variant == "step":
        ops.adam_step(pd, gd, md, vd, *args, step, grad_scale=gs)
        return pd, md, vd, pb
    if variant == "dev":
        ops.adam_step_dev(pd, gd, md, vd, *args, cnt, grad_scale=gs)
    elif variant == "cast":
        ops.adam_step_dev_cast(pd, gd, md, vd, pb, *args, cnt, grad_scale=gs)
    elif variant == "cast_g16":
        ops.adam_step_dev_cast_g16(pd, gd, md, vd, pb, *args, cnt, grad_scale=gs)
    else:
        ops.adam_tick(cnt)
        assert int(cnt) == step, "adam_tick"
        ops.adam_step_dev_range(pd, gd, md, vd, pb, *args, cnt, grad_scale=gs)
    assert int(cnt) == step, f"{variant}: step counter"
    return pd, md, vd, pb


def _adam_rule(ops, dev, name, variant, n, step, gs, p0zero, offset=False):
    """p, m and v of one variant against fp64 (the bf16-gradient variants restate from the rounded gradient);
    n < 64: ceil(64 / n) independent draws compared as one vector."""
    ndraw = max(1, -(-64 // n))
    got, r64, r32 = [], [], []
    for i in range(ndraw):
        p, g, m, v, zero = _adam_inputs(n, step, p0zero, seed=7919 * i)
        g_in = g.to(torch.bfloat16).float() if "g16" in variant else g
        out = _adam_launch(ops, dev, variant, p, g, m, v, step, gs, offset)
        got.append([t.cpu() for t in out[:3]])
        r64.append(_adam_ref(torch.float64, p, g_in, m, v, step, gs))
        r32.append(_adam_ref(torch.float32, p, g_in, m, v, step, gs))
        for sl in zero:
            assert _same_bits(out[0][sl], p[sl]) and not bool(out[1][sl].any()) and not bool(out[2][sl].any()), \
                "zero gradient on zero moments must leave p, m, v as they are"
        if out[3] is not None:
            assert _same_bits(out[3], out[0].to(torch.bfloat16)), f"{name}: p_bf16 != p.to(bfloat16)"
    for j, part in enumerate(("p", "m", "v")):
        _check(f"{name} {part}", torch.cat([t[j] for t in got]), torch.cat([t[j] for t in r64]),
               torch.cat([t[j] for t in r32]))


ADAM_SMALL = [  # n, step, grad_scale, p0 = 0
    (1, 1, 1.0, True), (3, 10, 0.5, False), (4, 1000, 1.0, False), (5, 1, 0.5, True),
    (1023, 1, 1.0, True), (1023, 10, 0.5, False), (1023, 1000, 1.0, False),
]


@pytest.mark.parametrize("variant", ADAM_VARIANTS)
@pytest.mark.parametrize("n,step,gs,p0zero", ADAM_SMALL, ids=[f"n{c[0]}_step{c[1]}" for c in ADAM_SMALL])
def test_adam_small(n, step, gs, p0zero, variant, dev):
    """Every entry point at n = 1, 3, 4, 5 (no float4 group, one group, a group and a tail element) and 1023, steps
    1 / 10 / 1000, grad_scale 0.5, p0 = 0 at step 1 (the update itself is what is measured)."""
    from vidsitu_amd import ops

    _adam_rule(ops, dev, f"adam_{variant} n={n} step={step} gs={gs}", variant, n, step, gs, p0zero)


@pytest.mark.parametrize("variant", ADAM_VARIANTS)
def test_adam_unaligned_views_take_the_scalar_tail(variant, dev):
    """p / m / v one float and the gradient and bf16 copy one element into their buffers (`_view` asserts it): n4 = 0,
    every element goes through the scalar tail."""
    from vidsitu_amd import ops

    _adam_rule(ops, dev, f"adam_{variant} n=1023 step=10 gs=0.5 unaligned", variant, 1023, 10, 0.5, False, offset=True)


def test_adam_betas_arrive_as_floats(dev):
    """What the float ABI costs against an Adam whose betas are the doubles 0.9 and 0.99 (torch.optim.Adam), at step 1
    from zero moments, where m = (1 - b1) g and v = (1 - b2) g^2: the kernel's 1 - 0.9f and 1 - 0.99f are exact
    differences of the rounded betas, off by d1 = 2.4e-7 and d2 = 9.5e-7 relative, and m and v carry exactly that:
    bound 16 * e32 + d.  p is printed, not asserted here: its bias corrections are formed from the same rounded
    betas, so the two deviations cancel in m / bc1 and sqrt(v / bc2) at step 1."""
    from vidsitu_amd import ops

    n, step = 1023, 1
    p, g, m, v, _ = _adam_inputs(n, step, True)
    out = _adam_launch(ops, dev, "dev", p, g, m, v, step, 1.0)
    r64 = _adam_ref(torch.float64, p, g, m, v, step, 1.0, ADAM_DOUBLES)
    r32 = _adam_ref(torch.float32, p, g, m, v, step, 1.0, ADAM_DOUBLES)
    for j, (part, exact, rounded) in enumerate((("p", None, None), ("m", 0.9, B1), ("v", 0.99, B2))):
        e32, err = _errs(out[j], r64[j], r32[j])
        d = 0.0 if exact is None else abs((1 - rounded) - (1 - exact)) / (1 - exact)
        print(f"PARITY adam_dev n={n} step={step} [betas as doubles] {part} e32={e32:.3e} err={err:.3e} d={d:.3e}")
        if exact is not None:
            assert d < 1e-6 and err <= FACTOR * e32 + d, part


ADAM_LARGE = [  # n, step, grad_scale
    (4194304, 1, 1.0),    # the full grid of 4096 x 256 threads, one float4 group each: `two` is false everywhere
    (4194327, 10, 0.5),   # five threads take a second group, three elements of scalar tail
    (8389809, 1000, 1.0),  # second trip of the loop for some threads (n / 4 > 2 * 4096 * 256), one tail element
]


@pytest.mark.parametrize("n,step,gs", ADAM_LARGE, ids=[f"n{c[0]}" for c in ADAM_LARGE])
def test_adam_large(n, step, gs, dev):
    """`adam_step` and `adam_step_dev` against fp64 where `adam_dev_kernel` takes its second float4 group and its
    second loop trip; the other entry points bit for bit: `_cast` == `_dev` followed by `cast_bf16`, `_range` after
    `adam_tick` == `_dev` (and `_range` leaves the counter alone: asserted in `_adam_launch`), the bf16-gradient
    variants == the fp32 ones fed `g16.float()`, p_bf16 == p.to(bfloat16)."""
    from vidsitu_amd import ops

    p, g, m, v, zero = _adam_inputs(n, step, step == 1)
    r64 = _adam_ref(torch.float64, p, g, m, v, step, gs)
    r32 = _adam_ref(torch.float32, p, g, m, v, step, gs)
    outs = {}
    for variant in ("step", "dev"):
        outs[variant] = _adam_launch(ops, dev, variant, p, g, m, v, step, gs)
        for j, part in enumerate(("p", "m", "v")):
            _check(f"adam_{variant} n={n} step={step} gs={gs} {part}", outs[variant][j], r64[j], r32[j])
        for sl in zero:
            assert _same_bits(outs[variant][0][sl], p[sl]) and not bool(outs[variant][1][sl].any())
    del r64, r32
    dev_p, dev_m, dev_v, _ = outs["dev"]
    ref_pb = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    ops.cast_bf16(dev_p, ref_pb)
    assert _same_bits(ref_pb, dev_p.to(torch.bfloat16)), "cast_bf16 != torch's cast"
    for variant in ("cast", "range", "range_pb"):
        pd, md, vd, pb = _adam_launch(ops, dev, variant, p, g, m, v, step, gs)
        assert _same_bits(pd, dev_p) and _same_bits(md, dev_m) and _same_bits(vd, dev_v), f"{variant} != dev"
        assert pb is None or _same_bits(pb, ref_pb), f"{variant}: p_bf16"
    g16 = g.to(torch.bfloat16)
    f_p, f_m, f_v, _ = _adam_launch(ops, dev, "dev", p, g16.float(), m, v, step, gs)
    for variant in ("cast_g16", "range_g16", "range_g16_pb"):
        pd, md, vd, pb = _adam_launch(ops, dev, variant, p, g, m, v, step, gs)
        assert _same_bits(pd, f_p) and _same_bits(md, f_m) and _same_bits(vd, f_v), f"{variant} != dev on g16.float()"
        assert pb is None or _same_bits(pb, f_p.to(torch.bfloat16)), f"{variant}: p_bf16"


def _f32_from_bits(words):
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32).view(torch.float32)


def _cast(ops, dev, x):
    out = torch.full((x.numel(),), -1.0, dtype=torch.bfloat16, device=dev)
    ops.cast_bf16(x.to(dev), out)
    return out.cpu()


def test_cast_f32_to_bf16_table(dev):
    """Bit for bit torch's cast: +-0, +-inf, ties to even in both directions and both signs, the neighbours of a tie,
    the largest finite float (rounds to inf), random normals; NaN stays NaN."""
    from vidsitu_amd import ops

    table = _f32_from_bits([
        0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
        0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,   # exactly between two bf16: down to even, up to even
        0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,   # just below / above a tie
        0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000,   # largest finite: inf; largest that stays finite; tie to inf
        0x00800000, 0x3F800000, 0x3F7FFFFF, 0x477FE000,
    ])
    x = torch.cat([table, torch.randn(1000, generator=_gen(1)), torch.randn(1000, generator=_gen(2)) * 1e-20,
                   torch.randn(1000, generator=_gen(3)) * 1e20])
    assert _same_bits(_cast(ops, dev, x), x.to(torch.bfloat16))
    nan = _f32_from_bits([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7F80FFFF])
    assert bool(torch.isnan(_cast(ops, dev, nan).float()).all()), "NaN in must give NaN out"


@pytest.mark.parametrize("n", [1, 1048577])
def test_cast_f32_to_bf16_sizes(n, dev):
    """n = 1 and the grid-stride loop (n > 4096 * 256)."""
    from vidsitu_amd import ops

    x = torch.randn(n, generator=_gen(n))
    assert _same_bits(_cast(ops, dev, x), x.to(torch.bfloat16))


def test_cast_f32_to_bf16_denormals(dev):
    """fp32 denormals (and the bf16-denormal range just above them): printed; the result is torch's or a signed zero."""
    from vidsitu_amd import ops

    x = _f32_from_bits([0x00000001, 0x00008000, 0x00010000, 0x00018000, 0x007FFFFF, 0x80000001, 0x80018000,
                        0x807FFFFF, 0x00400000, 0x80400000])
    got, want = _cast(ops, dev, x), x.to(torch.bfloat16)
    gb, wb = _bits(got).tolist(), _bits(want).tolist()
    for xi, a, b in zip(_bits(x).tolist(), gb, wb):
        print(f"PARITY cast_bf16 denormal in=0x{xi & 0xFFFFFFFF:08x} kernel=0x{a & 0xFFFF:04x} "
              f"torch=0x{b & 0xFFFF:04x}")
    for xi, a, b in zip(_bits(x).tolist(), gb, wb):
        zero = -32768 if xi < 0 else 0
        assert a == b or a == zero, f"0x{xi & 0xFFFFFFFF:08x} -> 0x{a & 0xFFFF:04x}"
