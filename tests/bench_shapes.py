"""The convolution geometries of one bench step (SlowFast-R50, N clips x 32 x 224^2), derived from the oracle's module
tree, and the reference arithmetic the bench-shape sweep holds the HIP kernels to (tests/test_gpu_conv_bench_shapes.py;
the helpers themselves are tested on the CPU by tests/test_bench_shapes.py).

The reference is the definition of the operation written as a loop over the kernel's taps -- each tap one strided slice
and one fp64 matrix product -- and calls no convolution routine of any library.  It runs on whichever device its
operands are on."""
import itertools
from collections import namedtuple

import torch

Row = namedtuple("Row", "name names count n cin t h w cout k s p")


def out_size(i, k, s, p):
    return (i + 2 * p - k) // s + 1


def row_out(r):
    """(To, Ho, Wo) of a row."""
    return tuple(out_size(i, k, s, p) for i, k, s, p in zip((r.t, r.h, r.w), r.k, r.s, r.p))


def row_positions(r):
    to, ho, wo = row_out(r)
    return r.n * to * ho * wo


def row_k(r):
    """Reduction length of the forward product."""
    return r.cin * r.k[0] * r.k[1] * r.k[2]


def row_macs(r):
    return row_positions(r) * r.cout * row_k(r)


def _walk(model, inputs):
    """[(module name, (Cin, T, H, W, Cout, k, s, p))] of every Conv3d, in call order."""
    seen, hooks = [], []

    def mk(name):
        def hook(m, inp, out):
            x = inp[0]
            seen.append((name, (m.in_channels, x.shape[2], x.shape[3], x.shape[4], m.out_channels,
                                tuple(m.kernel_size), tuple(m.stride), tuple(m.padding))))
        return hook

    for name, m in model.named_modules():
        if isinstance(m, torch.nn.Conv3d):
            hooks.append(m.register_forward_hook(mk(name)))
    with torch.no_grad():
        model.forward_features(list(inputs))
    for h in hooks:
        h.remove()
    return seen


def oracle_trunk_on_meta(frames=32):
    from oracle.slowfast_ref import VideoTrunk, default_sf_cfg

    cfg = default_sf_cfg("slowfast", 50, 64, frames)
    with torch.device("meta"):
        return VideoTrunk(cfg), cfg


def oracle_conv_list(n=8, hw=224, frames=32):
    """Every Conv3d call of the oracle's SlowFast-R50 on n clips of frames x hw x hw, walked on the meta device."""
    model, cfg = oracle_trunk_on_meta(frames)
    slow = torch.empty(n, 3, frames // cfg.SLOWFAST.ALPHA, hw, hw, device="meta")
    fast = torch.empty(n, 3, frames, hw, hw, device="meta")
    return _walk(model, [slow, fast])


def bench_rows(n=8, hw=224, frames=32):
    """The distinct (Cin, T, H, W, Cout, k, s, p) rows of the step, first-seen order, with the layers that share each."""
    groups = {}
    for name, key in oracle_conv_list(n, hw, frames):
        groups.setdefault(key, []).append(name)
    return [Row(names[0], tuple(names), len(names), n, *key) for key, names in groups.items()]


def product_conv_geometry(frames=32):
    """{module name: (Cin, Cout, k, s, p)} of the product's own trunk.  Needs no GPU: only the constructor runs."""
    from oracle.slowfast_ref import default_sf_cfg
    from vidsitu_amd.trunk import Conv3dP, VideoTrunk

    model = VideoTrunk(default_sf_cfg("slowfast", 50, 64, frames))
    return {name: (m.cin, m.cout, tuple(m.k), tuple(m.s), tuple(m.p))
            for name, m in model.named_modules() if isinstance(m, Conv3dP)}


def is_stem(r):
    """The rows the trunk runs on the dedicated stem kernels (vidsitu_amd.trunk.Conv3dP.is_stem)."""
    return r.cin == 3 and r.k[1:] == (7, 7) and r.s == (1, 2, 2) and r.p == (r.k[0] // 2, 3, 3)


# ----------------------------------------------------------------------------
# reference arithmetic: fp64, tap by tap
# ----------------------------------------------------------------------------
def _taps(k):
    return itertools.product(range(k[0]), range(k[1]), range(k[2]))


def _cl64(x):
    """logical [N, C, T, H, W] -> fp64 [N, T, H, W, C]."""
    return x.permute(0, 2, 3, 4, 1).to(torch.float64)


def _padded(xc, p):
    n, t, h, w, c = xc.shape
    xp = xc.new_zeros((n, t + 2 * p[0], h + 2 * p[1], w + 2 * p[2], c))
    xp[:, p[0]:p[0] + t, p[1]:p[1] + h, p[2]:p[2] + w] = xc
    return xp


def _tap_view(xp, tap, osz, s):
    """The (padded) input elements that tap (a, b, c) pairs with the outputs: padded[o * s + tap]."""
    return xp[:, tap[0]:tap[0] + (osz[0] - 1) * s[0] + 1:s[0],
              tap[1]:tap[1] + (osz[1] - 1) * s[1] + 1:s[1],
              tap[2]:tap[2] + (osz[2] - 1) * s[2] + 1:s[2]]


def conv_ref64(x, w, s, p):
    """y[n, o, t, i, j] = sum over taps (a, b, c) and channels ci of x[n, ci, t sT + a - pT, i sH + b - pH, j sW + c - pW]
    * w[o, ci, a, b, c]; fp64, logical [N, Cout, To, Ho, Wo]."""
    k = tuple(w.shape[2:])
    xp = _padded(_cl64(x), p)
    wd = w.to(torch.float64)
    osz = tuple(out_size(i, kk, ss, pp) for i, kk, ss, pp in zip(x.shape[2:], k, s, p))
    y = xp.new_zeros((x.shape[0], *osz, w.shape[0]))
    y2 = y.view(-1, w.shape[0])
    for tap in _taps(k):
        y2.addmm_(_tap_view(xp, tap, osz, s).reshape(-1, x.shape[1]), wd[:, :, tap[0], tap[1], tap[2]].t())
    return y.permute(0, 4, 1, 2, 3)


def dgrad_ref64(dy, w, xs, s, p):
    """dx[xs], the transpose of conv_ref64 in x: every tap adds dy . w[:, :, tap] onto the inputs it read."""
    k = tuple(w.shape[2:])
    n, cin, t, h, wi = xs
    wd = w.to(torch.float64)
    dyc = _cl64(dy)
    osz = tuple(dyc.shape[1:4])
    dy2 = dyc.reshape(-1, dyc.shape[4])
    dxp = dyc.new_zeros((n, t + 2 * p[0], h + 2 * p[1], wi + 2 * p[2], cin))
    for tap in _taps(k):
        _tap_view(dxp, tap, osz, s).add_(torch.matmul(dy2, wd[:, :, tap[0], tap[1], tap[2]]).view(n, *osz, cin))
    return dxp[:, p[0]:p[0] + t, p[1]:p[1] + h, p[2]:p[2] + wi].permute(0, 4, 1, 2, 3)


def wgrad_ref64(dy, x, k, s, p):
    """dw[o, ci, tap] = sum over output positions of dy[., o] * x[. s + tap - p, ci]; fp64, [Cout, Cin, kT, kH, kW].
    (One product per output frame, summed: a single [Cout x 3.2 million] x [3.2 million x 3] product of the fast stem
    runs on a handful of workgroups and takes 0.1 s per tap.)"""
    xp = _padded(_cl64(x), p)
    dyc = _cl64(dy)
    osz = tuple(dyc.shape[1:4])
    frames = dyc.shape[0] * osz[0]
    dy3t = dyc.reshape(frames, -1, dyc.shape[4]).transpose(1, 2)
    dw = xp.new_zeros((dy.shape[1], x.shape[1], *k))
    for tap in _taps(k):
        xv = _tap_view(xp, tap, osz, s).reshape(frames, -1, x.shape[1])
        dw[:, :, tap[0], tap[1], tap[2]] = torch.matmul(dy3t, xv).sum(0)
    return dw


def mag64(fn, a, w, *rest):
    """The same loop on |a|, |w| (fn = conv_ref64 or dgrad_ref64): the sum of |products| behind every output, the scale
    of an fp32 accumulation's rounding error."""
    return fn(a.abs(), w.abs(), *rest)


def rel_l2_64(got, ref):
    got, ref = got.to(torch.float64), ref.to(torch.float64)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def rb64(x):
    """fp64 -> bf16 -> fp64.  (Through fp32: the double rounding can only differ from a direct one within 2^-29 relative
    of a bf16 tie, where either neighbour is half an ulp away: the distance to `x` is the same.)"""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)
