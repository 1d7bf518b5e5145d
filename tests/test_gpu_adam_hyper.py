"""The Adam entry point that reads its hyper-parameters from device memory (`vs_adam_step_hp`) and the gradient-norm
pass in front of it (`vs_grad_sumsq`), csrc/txenc_ops.hip.

The specification is torch itself: `torch.optim.Adam`, `torch.optim.AdamW` and `torch.nn.utils.clip_grad_norm_` run on
CPU tensors in fp64.  Tolerance, the rule of tests/test_gpu_txenc_ops.py: the same torch run in fp32 gives the
restatement's own noise floor `e32` (max |diff| / max |fp64|); the kernel's error, measured the same way, is at most
min(16 * e32, 2e-4).  Every figure is printed (`PARITY ...`) before it is asserted; bitwise claims are compared on the
bits.  The norm and the clip coefficient have a bound of their own, 4 * 2^-24 relative: the kernel accumulates fewer
than 2^27 squares in fp64 (error below 2^-26), and the square root, the scale and the rounding to fp32 add at most
2^-24; the coefficient is one more fp32 add and one fp32 divide on top of the rounded norm (3 * 2^-24 in all).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FACTOR = 16.0
CEILING = 2e-4
NORM_BOUND = 4 * 2.0 ** -24
CHUNK = 2048  # the norm pass's smallest partial (VS_SUMSQ_ALIGN): sizes around its multiples turn the partition


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
    return min(FACTOR * e32, CEILING)


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


# The C ABI takes betas and eps as floats and the hyper block is float32: they enter torch as those values, promoted.
LR, B1, B2, EPS = (_f32(c) for c in (1e-3, 0.9, 0.99, 1e-8))
LR_BIG, WD = _f32(1e-2), _f32(0.1)


def _view(t, dev, offset):
    """t on the device; with `offset` as a view one element into a larger buffer (no 16-byte / 8-byte alignment)."""
    if not offset:
        return t.to(dev)
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=dev)
    view = buf[1:1 + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


def _inputs(n, step0, nsteps=1, seed=0):
    """p, m, v before step `step0 + 1` and one gradient per step."""
    g = _gen(n * 31 + step0 + seed)
    p = torch.randn(n, generator=g)
    if step0 == 0:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m, v = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
    return p, m, v, [torch.randn(n, generator=g) for _ in range(nsteps)]


def _torch_ref(dt, p, m, v, grads, step0, gs, lrs, wd=0.0, decoupled=False, max_norm=None):
    """One torch optimizer step per gradient from step count `step0`: clip_grad_norm_ (when max_norm), then
    torch.optim.Adam / AdamW -> p, m, v, [norm per step], [coefficient per step]."""
    q = torch.nn.Parameter(p.to(dt).clone())
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([q], lr=lrs[0], betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    if step0 > 0:
        opt.state[q] = {"step": torch.tensor(float(step0)), "exp_avg": m.to(dt).clone(),
                        "exp_avg_sq": v.to(dt).clone()}
    norms, coefs = [], []
    for lr, g in zip(lrs, grads):
        opt.param_groups[0]["lr"] = lr
        q.grad = g.to(dt) * gs
        if max_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_([q], max_norm, foreach=False)
            norms.append(float(norm))
            coefs.append(min(1.0, max_norm / (float(norm) + 1e-6)))
        opt.step()
    st = opt.state[q]
    return q.detach(), st["exp_avg"], st["exp_avg_sq"], norms, coefs


class _Dev:
    """Device-side state of one optimizer: p, m, v (+ bf16 copy), the step counter, the hyper block, the workspace."""

    def __init__(self, ops, dev, p, m, v, step0, g16=False, with_pb=False, offset=False, lr=LR, wd=0.0, max_norm=0.0,
                 clip=False):
        self.ops, self.dev, self.g16, self.offset = ops, dev, g16, offset
        self.p, self.m, self.v = (_view(t.clone(), dev, offset) for t in (p, m, v))
        self.pb = _view(torch.zeros(p.numel(), dtype=torch.bfloat16), dev, offset) if with_pb else None
        self.cnt = torch.tensor([step0], dtype=torch.int32, device=dev)
        self.hyper = torch.tensor([lr, wd, max_norm, 0, 0, 0, 0, 0], dtype=torch.float32, device=dev)
        self.ws = ops.grad_sumsq_workspace(p.numel(), dev) if clip else None

    def grad(self, g):
        return _view(g.to(torch.bfloat16) if self.g16 else g, self.dev, self.offset)

    def step(self, g, gs=1.0, tick=True, decoupled=False):
        gd = self.grad(g)
        if self.ws is not None:
            self.ops.grad_sumsq(gd, self.ws)
        if not tick:
            self.ops.adam_tick(self.cnt)
        self.ops.adam_step_hp(self.p, gd, self.m, self.v, self.pb, self.hyper, B1, B2, EPS, self.cnt, tick=tick,
                              grad_scale=gs, decoupled=decoupled, sumsq_ws=self.ws)
        return self

    def out(self):
        return [self.p.cpu(), self.m.cpu(), self.v.cpu(), None if self.pb is None else self.pb.cpu(), int(self.cnt)]


def _existing(ops, dev, p, g, m, v, step0, gs, g16, with_pb, tick, offset):
    """The same update through the entry points that exist without the hyper block."""
    pd, md, vd = (_view(t.clone(), dev, offset) for t in (p, m, v))
    gd = _view(g.to(torch.bfloat16) if g16 else g, dev, offset)
    pb = _view(torch.zeros(p.numel(), dtype=torch.bfloat16), dev, offset) if with_pb else None
    cnt = torch.tensor([step0], dtype=torch.int32, device=dev)
    if tick and not g16 and not with_pb:
        ops.adam_step_dev(pd, gd, md, vd, LR, B1, B2, EPS, cnt, grad_scale=gs)
    elif tick and not g16:
        ops.adam_step_dev_cast(pd, gd, md, vd, pb, LR, B1, B2, EPS, cnt, grad_scale=gs)
    elif tick and with_pb:
        ops.adam_step_dev_cast_g16(pd, gd, md, vd, pb, LR, B1, B2, EPS, cnt, grad_scale=gs)
    else:
        ops.adam_tick(cnt)
        ops.adam_step_dev_range(pd, gd, md, vd, pb, LR, B1, B2, EPS, cnt, grad_scale=gs)
    return [pd.cpu(), md.cpu(), vd.cpu(), None if pb is None else pb.cpu(), int(cnt)]


def _assert_same(name, got, want):
    for part, a, b in zip(("p", "m", "v", "p_bf16"), got, want):
        assert (a is None) == (b is None), f"{name}: {part}"
        assert a is None or _same_bits(a, b), f"{name}: {part} differs in its bits"
    assert got[4] == want[4], f"{name}: step count {got[4]} vs {want[4]}"


def _bitwise_case(ops, dev, n, step0, gs, g16, with_pb, tick, offset=False):
    p, m, v, (g,) = _inputs(n, step0)
    name = f"adam_hp n={n} g16={g16} pb={with_pb} tick={tick}"
    want = _existing(ops, dev, p, g, m, v, step0, gs, g16, with_pb, tick, offset)
    plain = _Dev(ops, dev, p, m, v, step0, g16, with_pb, offset).step(g, gs, tick)
    _assert_same(name + " [wd=0, no workspace]", plain.out(), want)
    armed = _Dev(ops, dev, p, m, v, step0, g16, with_pb, offset, max_norm=1e9, clip=True).step(g, gs, tick)
    _assert_same(name + " [clip armed, under the limit]", armed.out(), want)
    h = armed.hyper.cpu()
    assert float(h[4]) == 1.0 and float(h[3]) > 0, h
    assert want[4] == step0 + 1


SMALL = [(1, 0, 1.0, False), (3, 9, 0.5, False), (4, 999, 1.0, False), (5, 0, 0.5, False), (1023, 9, 0.5, True),
         (2049, 9, 0.5, False)]


@pytest.mark.parametrize("tick", [1, 0])
@pytest.mark.parametrize("with_pb", [False, True])
@pytest.mark.parametrize("g16", [False, True])
@pytest.mark.parametrize("n,step0,gs,offset", SMALL, ids=[f"n{c[0]}" for c in SMALL])
def test_default_hyper_is_bitwise_the_existing_kernels(n, step0, gs, offset, g16, with_pb, tick, dev):
    """n = 1, 3, 4, 5 (no float4 group, one, one and a tail), 1023 on an unaligned view (scalar loop only), 2049 (more
    than one block): wd = 0 without a workspace, and with an armed clip whose limit is not reached, are the existing
    entry points bit for bit -- p, m, v, the bf16 copy and the step count."""
    from vidsitu_amd import ops

    _bitwise_case(ops, dev, n, step0, gs, g16, with_pb, bool(tick), offset)


@pytest.mark.parametrize("g16,with_pb,tick", [(False, True, 1), (True, False, 0)], ids=["f32_pb_tick", "g16_range"])
def test_default_hyper_is_bitwise_the_existing_kernels_large(g16, with_pb, tick, dev):
    """n = 8 389 809: the second float4 group and the second trip of the grid-stride loop, one tail element."""
    from vidsitu_amd import ops

    _bitwise_case(ops, dev, 8389809, 999, 1.0, g16, with_pb, bool(tick))


# ---------------------------------------------------------------------------------------------
# the norm
# ---------------------------------------------------------------------------------------------
NORM_CASES = [  # n, bf16, grad_scale, unaligned view, index of a 1e30 element
    (1, False, 1.0, False, None), (3, True, 0.5, False, None), (255, False, 0.5, False, None),
    (CHUNK - 1, False, 1.0, False, None), (CHUNK + 1, True, 1.0, False, None),
    (3 * CHUNK - 1, True, 0.5, True, None), (3 * CHUNK + 1, False, 0.5, True, None),
    (5 * CHUNK + 1, False, 1.0, False, 4099),
    (8389809, False, 0.5, False, None), (8389809, True, 1.0, False, None),
]


@pytest.mark.parametrize("n,g16,gs,offset,big", NORM_CASES,
                         ids=[f"n{c[0]}_{'bf16' if c[1] else 'f32'}{'_1e30' if c[4] is not None else ''}" for c in NORM_CASES])
def test_grad_norm_against_fp64(n, g16, gs, offset, big, dev):
    """hyper[3] against float32(grad_scale * sqrt(fp64 sum of squares)) within 4 * 2^-24, at sizes around the
    partition's turns, on aligned and unaligned views, and with one 1e30 element (its square overflows fp32)."""
    from vidsitu_amd import ops

    p, m, v, (g,) = _inputs(n, 0)
    if big is not None:
        g[big] = 1e30
    st = _Dev(ops, dev, p, m, v, 0, g16=g16, offset=offset, clip=True).step(g, gs)
    g_in = g.to(torch.bfloat16) if g16 else g
    want = _f32(gs * math.sqrt(float((g_in.double() ** 2).sum())))
    got = float(st.hyper[3])
    err = abs(got - want) / want
    print(f"PARITY grad_norm n={n} g16={g16} gs={gs} unaligned={offset} norm={want:.9e} err={err:.3e} bound={NORM_BOUND:.3e}")
    assert math.isfinite(got) and err <= NORM_BOUND
    assert float(st.hyper[4]) == 1.0  # max_grad_norm = 0: measured, not clipped
    part = st.ws.cpu()
    per = -(-n // 1024)
    chunk = -(-per // CHUNK) * CHUNK
    assert part.numel() == 1024 and not bool(part[-(-n // chunk):].any()), "partials past the end must be zero"


def test_nan_gradient_shows_in_the_norm(dev):
    from vidsitu_amd import ops

    p, m, v, (g,) = _inputs(5000, 0)
    g[4321] = float("nan")
    st = _Dev(ops, dev, p, m, v, 0, max_norm=1.0, clip=True).step(g)
    assert math.isnan(float(st.hyper[3]))


@pytest.mark.parametrize("g16", [False, True])
def test_same_launch_twice_is_bitwise_equal(g16, dev):
    """No atomics anywhere: norm, coefficient and every updated element repeat bit for bit."""
    from vidsitu_amd import ops

    p, m, v, (g,) = _inputs(1000003, 9)
    runs = [_Dev(ops, dev, p, m, v, 9, g16=g16, with_pb=True, wd=WD, max_norm=1.0, clip=True).step(g, 0.5)
            for _ in range(2)]
    _assert_same("twice", runs[0].out(), runs[1].out())
    assert _same_bits(runs[0].hyper, runs[1].hyper)
    assert torch.equal(runs[0].ws.cpu().view(torch.int64), runs[1].ws.cpu().view(torch.int64))
    assert float(runs[0].hyper[4]) < 1.0


# ---------------------------------------------------------------------------------------------
# clip, weight decay, device-read lr against torch in fp64
# ---------------------------------------------------------------------------------------------
def _parity(name, st, r64, r32):
    bounds = []
    for j, part in enumerate(("p", "m", "v")):
        bounds.append(_check(f"{name} {part}", (st.p, st.m, st.v)[j].cpu(), r64[j], r32[j]))
    if st.pb is not None:
        assert _same_bits(st.pb, st.p.to(torch.bfloat16)), f"{name}: p_bf16 != p.to(bfloat16)"
    return bounds


@pytest.mark.parametrize("n,g16,offset", [(2049, False, False), (1023, True, True), (67, False, False)],
                         ids=["n2049", "n1023_bf16_unaligned", "n67"])
def test_clip_above_the_limit(n, g16, offset, dev):
    """Three steps whose norm is above max_grad_norm (randn gradients: norm ~ sqrt(n) * grad_scale against 0.25):
    clip_grad_norm_ + torch.optim.Adam in fp64; the coefficient within 4 * 2^-24 of the fp64 one."""
    from vidsitu_amd import ops

    gs, max_norm, step0 = 0.5, 0.25, 9
    p, m, v, grads = _inputs(n, step0, 3)
    g_in = [g.to(torch.bfloat16).float() for g in grads] if g16 else grads
    r64 = _torch_ref(torch.float64, p, m, v, g_in, step0, gs, [LR] * 3, max_norm=max_norm)
    r32 = _torch_ref(torch.float32, p, m, v, g_in, step0, gs, [LR] * 3, max_norm=max_norm)
    st = _Dev(ops, dev, p, m, v, step0, g16=g16, with_pb=True, offset=offset, max_norm=max_norm, clip=True)
    for i, g in enumerate(grads):
        st.step(g, gs)
        norm, coef = float(st.hyper[3]), float(st.hyper[4])
        en, ec = abs(norm - r64[3][i]) / r64[3][i], abs(coef - r64[4][i]) / r64[4][i]
        print(f"PARITY clip n={n} step {i} norm={norm:.7e} err={en:.3e} coef={coef:.7e} err={ec:.3e} bound={NORM_BOUND:.3e}")
        assert coef < 1.0 and en <= NORM_BOUND and ec <= NORM_BOUND
    assert int(st.cnt) == step0 + 3
    _parity(f"adam_hp clip n={n} g16={g16}", st, r64, r32)


@pytest.mark.parametrize("n,g16,offset", [(2049, False, False), (1023, True, True)], ids=["n2049", "n1023_bf16_unaligned"])
def test_weight_decay_both_forms(n, g16, offset, dev):
    """torch.optim.Adam(weight_decay) -- g += wd * p -- and torch.optim.AdamW -- p *= 1 - lr * wd -- over three steps at
    wd = 0.1, lr = 1e-2: each form within the parity rule of its own torch run, and the two apart by more than it."""
    from vidsitu_amd import ops

    gs, step0 = 0.5, 0
    p, m, v, grads = _inputs(n, step0, 3)
    g_in = [g.to(torch.bfloat16).float() for g in grads] if g16 else grads
    got, bound = {}, {}
    for decoupled in (False, True):
        r64 = _torch_ref(torch.float64, p, m, v, g_in, step0, gs, [LR_BIG] * 3, wd=WD, decoupled=decoupled)
        r32 = _torch_ref(torch.float32, p, m, v, g_in, step0, gs, [LR_BIG] * 3, wd=WD, decoupled=decoupled)
        st = _Dev(ops, dev, p, m, v, step0, g16=g16, with_pb=True, offset=offset, lr=LR_BIG, wd=WD)
        for g in grads:
            st.step(g, gs, decoupled=decoupled)
        bound[decoupled] = _parity(f"adam_hp wd {'AdamW' if decoupled else 'L2'} n={n} g16={g16}", st, r64, r32)[0]
        got[decoupled] = (st.p.cpu(), r64[0])
    apart = float((got[False][0].double() - got[True][0].double()).abs().max()) / float(got[False][1].abs().max())
    print(f"PARITY adam_hp wd n={n} L2 vs AdamW apart={apart:.3e} bounds={bound[False]:.3e} {bound[True]:.3e}")
    assert apart > max(bound.values())


def test_lr_is_read_on_the_device_eager(dev):
    """Two launches with hyper[0] changed in between follow the fp64 run with both rates."""
    from vidsitu_amd import ops

    n, step0, lrs = 2049, 9, [LR, LR_BIG]
    p, m, v, grads = _inputs(n, step0, 2)
    r64 = _torch_ref(torch.float64, p, m, v, grads, step0, 1.0, lrs)
    r32 = _torch_ref(torch.float32, p, m, v, grads, step0, 1.0, lrs)
    st = _Dev(ops, dev, p, m, v, step0, with_pb=True, lr=lrs[0])
    st.step(grads[0])
    st.hyper[0:1].fill_(lrs[1])
    st.step(grads[1])
    _parity("adam_hp two rates, eager", st, r64, r32)
    one_rate = _torch_ref(torch.float64, p, m, v, grads, step0, 1.0, [LR, LR])
    assert float((one_rate[0] - r64[0]).abs().max()) / float(r64[0].abs().max()) > CEILING  # the rates are told apart


def test_lr_is_read_on_the_device_captured(dev):
    """One launch captured in a graph; replay, fill a new rate, replay: the fp64 run with both rates."""
    from vidsitu_amd import ops

    n, step0, lrs = 2049, 9, [LR, LR_BIG]
    p, m, v, (g,) = _inputs(n, step0)
    r64 = _torch_ref(torch.float64, p, m, v, [g, g], step0, 1.0, lrs)
    r32 = _torch_ref(torch.float32, p, m, v, [g, g], step0, 1.0, lrs)
    _Dev(ops, dev, p, m, v, step0, with_pb=True).step(g)  # the kernel is loaded before the capture
    st = _Dev(ops, dev, p, m, v, step0, with_pb=True, lr=lrs[0])
    gd = st.grad(g)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.adam_step_hp(st.p, gd, st.m, st.v, st.pb, st.hyper, B1, B2, EPS, st.cnt, tick=True)
    graph.replay()
    st.hyper[0:1].fill_(lrs[1])
    graph.replay()
    torch.cuda.synchronize()
    assert int(st.cnt) == step0 + 2
    _parity("adam_hp two rates, one captured launch", st, r64, r32)


def test_ranged_calls_share_the_whole_arena_norm(dev):
    """One tick and three ranged calls, each given its sub-range and the WHOLE arena's workspace, are one whole-arena
    call bit for bit (clip above the limit, weight decay on)."""
    from vidsitu_amd import ops

    n, step0, gs = 6151, 9, 0.5
    p, m, v, (g,) = _inputs(n, step0)
    for g16 in (False, True):
        kw = dict(g16=g16, with_pb=True, wd=WD, max_norm=0.25, clip=True)
        whole = _Dev(ops, dev, p, m, v, step0, **kw).step(g, gs)
        parts = _Dev(ops, dev, p, m, v, step0, **kw)
        gd = parts.grad(g)
        ops.grad_sumsq(gd, parts.ws)
        ops.adam_tick(parts.cnt)
        for lo, hi in ((0, 1024), (1024, 4100), (4100, n)):
            ops.adam_step_hp(parts.p[lo:hi], gd[lo:hi], parts.m[lo:hi], parts.v[lo:hi], parts.pb[lo:hi], parts.hyper,
                             B1, B2, EPS, parts.cnt, tick=False, grad_scale=gs, sumsq_ws=parts.ws)
        _assert_same(f"ranged g16={g16}", parts.out(), whole.out())
        assert _same_bits(parts.hyper, whole.hyper) and float(whole.hyper[4]) < 1.0
