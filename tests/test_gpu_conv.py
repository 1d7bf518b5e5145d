"""Parity of the HIP conv kernels (through the C-ABI) with fp32 torch conv3d on the same
bf16-rounded operands.  Tolerance: outputs are rounded to bf16 once (2^-9 relative) and
accumulated in fp32 in a different order, so 1e-2 of the tensor's max magnitude.
Covers every kernel family of SlowFast-R50, every tile config of
pick_tile(), K / M / N tails, strides, padding, the fused epilogue and the BN partials."""
import pytest
import torch
import torch.nn.functional as F

from gpu_utils import assert_close, rb, to_act, to_w
from partials_guard import guarded_partials  # noqa: F401  (the row-guard fixture, shared with test_gpu_stem_edges.py)
from vidsitu_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 1e-2

# name, N, Cin, T, H, W, Cout, k, s, p
CASES = [
    ("pw_64_256", 2, 64, 4, 14, 14, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("pw_k80_tail", 2, 80, 2, 12, 12, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("pw_8_32_fast", 1, 8, 4, 18, 18, 32, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("pw_32_8", 1, 32, 4, 18, 18, 8, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("pw_stride2", 2, 64, 2, 14, 14, 128, (1, 1, 1), (1, 2, 2), (0, 0, 0)),
    ("pw_320_512_s2", 1, 320, 2, 14, 14, 512, (1, 1, 1), (1, 2, 2), (0, 0, 0)),
    ("pw_bigM_128x128", 2, 16, 8, 64, 64, 128, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("pw_bigM_128x64", 2, 16, 8, 64, 64, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("t3_32_8", 2, 32, 8, 8, 8, 8, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    ("t3_256_64", 1, 256, 4, 7, 7, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    ("t3_640_256", 1, 640, 3, 6, 6, 256, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    ("s3_64_64", 2, 64, 2, 14, 14, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    ("s3_16_16_s2", 2, 16, 4, 14, 14, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("s3_8_8", 1, 8, 4, 20, 20, 8, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    ("s3_128_128", 1, 128, 2, 7, 7, 128, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    ("s3_odd_hw", 1, 32, 3, 9, 11, 32, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("fuse_7x1x1_s4", 2, 8, 32, 6, 6, 16, (7, 1, 1), (4, 1, 1), (3, 0, 0)),
    ("fuse_32_64", 1, 32, 16, 5, 5, 64, (7, 1, 1), (4, 1, 1), (3, 0, 0)),
    # small-channel layers of the fast pathway -> direct (register-resident weights) kernel
    ("dir_8_8_3x3_big", 2, 8, 8, 40, 40, 8, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    ("dir_32_8_t3", 1, 32, 16, 24, 24, 8, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    ("dir_8_32_pw", 2, 8, 8, 36, 36, 32, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("dir_16_16_s2", 2, 16, 6, 30, 26, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("dir_8_32_pw_s2", 1, 8, 4, 30, 30, 32, (1, 1, 1), (1, 2, 2), (0, 0, 0)),
    ("stem_slow", 1, 8, 2, 32, 32, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3)),
    ("stem_fast", 1, 8, 8, 32, 32, 8, (5, 7, 7), (1, 2, 2), (2, 3, 3)),
]


def _mk(case, seed=0):
    name, n, cin, t, h, w, cout, k, s, p = case
    g = torch.Generator().manual_seed(seed)
    x = rb(torch.randn(n, cin, t, h, w, generator=g))
    wt = rb(torch.randn(cout, cin, *k, generator=g) / (cin * k[0] * k[1] * k[2]) ** 0.5)
    return x, wt, k, s, p


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv_fwd_matches_torch(case, dev):
    from vidsitu_amd import ops

    x, w, k, s, p = _mk(case)
    ref = F.conv3d(x, w, stride=s, padding=p)
    y, _ = ops.conv_fwd(to_act(x, dev), to_w(w, dev), k, s, p)
    assert tuple(y.shape) == tuple(ref.shape)
    assert_close(y, ref, TOL, case[0])


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[9], CASES[12], CASES[16], CASES[18], CASES[24]],
                         ids=lambda c: c[0])
def test_mfma_kernel_matches_naive_hip_kernel(case, dev):
    """Two independent HIP implementations of the same gather agree (isolates MFMA/LDS bugs)."""
    from vidsitu_amd import ops

    x, w, k, s, p = _mk(case, seed=3)
    xa, wa = to_act(x, dev), to_w(w, dev)
    y1, _ = ops.conv_fwd(xa, wa, k, s, p)
    y2, _ = ops.conv_fwd(xa, wa, k, s, p, naive=True)
    assert_close(y1, y2.float(), 8e-3, case[0])


def test_conv_fused_epilogue_and_concat_write(dev):
    """scale/shift + residual + ReLU, written into a channel slice of a wider buffer and
    read from one (the FuseFastToSlow in-place concat)."""
    from vidsitu_amd import ops

    g = torch.Generator().manual_seed(1)
    n, cin, cout, t, h, w = 2, 64, 64, 2, 10, 10
    xfull = rb(torch.randn(n, cin + 16, t, h, w, generator=g))
    wt = rb(torch.randn(cout, cin, 1, 3, 3, generator=g) / 24.0)
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    res = rb(torch.randn(n, cout, t, h, w, generator=g))
    ref = F.relu(F.conv3d(xfull[:, 16:], wt, padding=(0, 1, 1)) * scale.view(1, -1, 1, 1, 1)
                 + shift.view(1, -1, 1, 1, 1) + res)
    xa = to_act(xfull, dev)[:, 16:]
    buf = ops.new_act(n, cout + 32, t, h, w, dev, zero=True)
    out = buf[:, 32:]
    ops.conv_fwd(xa, to_w(wt, dev), (1, 3, 3), (1, 1, 1), (0, 1, 1), out=out,
                 scale=scale.to(dev), shift=shift.to(dev), residual=to_act(res, dev), relu=True)
    assert_close(buf[:, 32:], ref, TOL, "fused epilogue")
    assert float(buf[:, :32].float().abs().max()) == 0.0  # neighbours untouched


@pytest.mark.parametrize("case", [CASES[1], CASES[7], CASES[10], CASES[11], CASES[13], CASES[14], CASES[17],
                                  CASES[18], CASES[20], CASES[21]], ids=lambda c: c[0])
def test_conv_bn_stat_partials(case, dev, guarded_partials):
    from vidsitu_amd import ops

    x, w, k, s, p = _mk(case, seed=5)
    ref = F.conv3d(x, w, stride=s, padding=p)
    y, partials = ops.conv_fwd(to_act(x, dev), to_w(w, dev), k, s, p, stats=True)
    tot = partials.double().sum(0).cpu()
    rsum = ref.double().sum(dim=(0, 2, 3, 4))
    rsq = (ref.double() ** 2).sum(dim=(0, 2, 3, 4))
    assert torch.allclose(tot[0], rsum, rtol=1e-3, atol=1e-3 * float(ref.abs().max()) * 10)
    assert torch.allclose(tot[1], rsq, rtol=1e-3, atol=1e-3)


DG_CASES = [CASES[i] for i in (0, 1, 3, 4, 5, 8, 9, 11, 12, 14, 15, 16, 17, 18, 19, 20, 21, 22)]


@pytest.mark.parametrize("case", DG_CASES, ids=[c[0] for c in DG_CASES])
def test_conv_dgrad_matches_autograd(case, dev):
    from vidsitu_amd import ops

    x, w, k, s, p = _mk(case, seed=7)
    x.requires_grad_()
    y = F.conv3d(x, w, stride=s, padding=p)
    dy = rb(torch.randn(y.shape, generator=torch.Generator().manual_seed(9)))
    (dx_ref,) = torch.autograd.grad(y, x, dy)
    wt = ops.weight_transpose(to_w(w, dev))
    dx = ops.conv_dgrad(to_act(dy, dev), wt, tuple(x.shape), k, s, p)
    assert_close(dx, dx_ref, TOL, case[0])
    dxn = ops.conv_dgrad(to_act(dy, dev), wt, tuple(x.shape), k, s, p, naive=True)
    assert_close(dxn, dx_ref, TOL, case[0] + " naive")
    # fan-out accumulation: dx = dgrad + residual (may alias the output)
    r = rb(torch.randn(x.shape, generator=torch.Generator().manual_seed(11)))
    ra = to_act(r, dev)
    ops.conv_dgrad(to_act(dy, dev), wt, tuple(x.shape), k, s, p, out=ra, residual=ra)
    assert_close(ra, dx_ref + r, TOL, case[0] + " +residual in place")


WG_CASES = [CASES[i] for i in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 19, 21, 23, 24)]


@pytest.mark.parametrize("case", WG_CASES, ids=[c[0] for c in WG_CASES])
def test_conv_wgrad_matches_autograd(case, dev):
    from vidsitu_amd import ops

    x, w, k, s, p = _mk(case, seed=13)
    w.requires_grad_()
    y = F.conv3d(x, w, stride=s, padding=p)
    dy = rb(torch.randn(y.shape, generator=torch.Generator().manual_seed(15)))
    (dw_ref,) = torch.autograd.grad(y, w, dy)
    dw = ops.conv_wgrad(to_act(dy, dev), to_act(x, dev), k, s, p)
    assert tuple(dw.shape) == tuple(dw_ref.shape)
    assert_close(dw, dw_ref, 5e-3, case[0])  # fp32 output, only operand rounding differs


# name, N, Cin, T, H, W, Cout, k, s, p: weight gradients for the deep-pipeline kernel (128 x 256 output tiles)
WGD_CASES = [
    ("s4a_t3_1024_256", 2, 1024, 8, 14, 14, 256, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    ("s4b_3x3_256", 2, 256, 8, 14, 14, 256, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    ("pw_1024_512", 2, 1024, 4, 14, 14, 512, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("pw_strided_640_1024", 2, 640, 4, 14, 14, 1024, (1, 1, 1), (1, 2, 2), (0, 0, 0)),
    ("3x3_strided_256_256", 2, 256, 4, 14, 14, 256, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("ragged_72_136", 3, 72, 3, 13, 11, 136, (1, 3, 3), (1, 1, 1), (0, 1, 1)),   # Cout 128 + 8, K' 648 = 2 x 256 + 136, P = 1287
    ("short_64_128", 1, 64, 2, 9, 9, 128, (1, 3, 3), (1, 1, 1), (0, 1, 1)),        # 162 positions: 6 units (< the 6-slot ring + 1)
    ("one_unit_64_128", 1, 64, 1, 5, 6, 128, (1, 1, 1), (1, 1, 1), (0, 0, 0)),     # 30 positions: a single, partial unit
    ("long_128_128", 4, 128, 16, 14, 14, 128, (3, 1, 1), (1, 1, 1), (1, 0, 0)),    # 12 544 positions: table chunks rebuilt in flight
    ("t5_64_320", 2, 64, 8, 9, 9, 320, (5, 1, 1), (1, 1, 1), (2, 0, 0)),
]


@pytest.mark.parametrize("case", WGD_CASES, ids=[c[0] for c in WGD_CASES])
def test_deep_pipeline_wgrad_matches_autograd_and_the_ring_kernel(case, dev):
    """conv_wgrad_deep_kernel (128 x 256 tile, units of 32 positions, six-slot ring, five units in flight): against
    autograd on the same bf16 operands, against fp64 at the kernel's own accuracy, against the ring kernel, and run to
    run bit for bit -- pointwise dense / strided, temporal and spatial taps, ragged Cout / K' / position counts,
    position ranges shorter than the ring and longer than a table chunk."""
    from vidsitu_amd import ops

    name, n, cin, t, h, w, cout, k, s, p = case
    g = torch.Generator().manual_seed(91)
    x = rb(torch.randn(n, cin, t, h, w, generator=g))
    wgt = torch.zeros(cout, cin, *k, requires_grad=True)
    y = F.conv3d(x, wgt, stride=s, padding=p)
    dy = rb(torch.randn(y.shape, generator=g))
    (dw_ref,) = torch.autograd.grad(y, wgt, dy)
    xa, dya = to_act(x, dev), to_act(dy, dev)
    dw = ops.conv_wgrad(dya, xa, k, s, p, deep="force")
    assert tuple(dw.shape) == tuple(dw_ref.shape)
    assert_close(dw, dw_ref, 5e-3, name)
    # fp64 on the same operands: only the kernel's own arithmetic is left
    w64 = torch.zeros(cout, cin, *k, dtype=torch.float64, device=dev, requires_grad=True)
    ref64 = torch.autograd.grad(F.conv3d(x.to(dev).double(), w64, stride=s, padding=p), w64, dy.to(dev).double())[0]
    err = float((dw.double() - ref64).norm() / ref64.norm())
    assert err <= 5e-6, err
    dw0 = ops.conv_wgrad(dya, xa, k, s, p, deep=False)
    assert_close(dw, dw0.float(), 1e-5, name + " vs ring kernel")
    assert torch.equal(ops.conv_wgrad(dya, xa, k, s, p, deep="force"), dw)


def test_direct_kernel_epilogue_and_residual(dev):
    """The register-resident small-channel kernel: affine + ReLU, residual add (dgrad fan-out),
    forced tiled kernel gives the same answer."""
    from vidsitu_amd import ops

    x, w, k, s, p = _mk(CASES[18], seed=21)
    g = torch.Generator().manual_seed(22)
    cout = w.shape[0]
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    ref0 = F.conv3d(x, w, stride=s, padding=p)
    res = rb(torch.randn(ref0.shape, generator=g))
    ref = F.relu(ref0 * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1) + res)
    xa, wa = to_act(x, dev), to_w(w, dev)
    y, _ = ops.conv_fwd(xa, wa, k, s, p, scale=scale.to(dev), shift=shift.to(dev),
                        residual=to_act(res, dev), relu=True)
    assert_close(y, ref, TOL, "direct kernel: affine + residual + relu")
    y_tiled, _ = ops.conv_fwd(xa, wa, k, s, p, scale=scale.to(dev), shift=shift.to(dev),
                              residual=to_act(res, dev), relu=True, tile=5)
    assert_close(y, y_tiled.float(), 8e-3, "direct vs tiled kernel")


def test_splitk_path_epilogue(dev, guarded_partials):
    """Few-tile deep-K shapes take the split-K plan (fp32 slabs + fused reduce/epilogue kernel):
    affine + residual + ReLU + BN partials must match, and two runs must be bit-identical."""
    from vidsitu_amd import ops

    for case in (CASES[10], CASES[14]):  # t3_640_256 (S=3), s3_128_128 (S=2)
        x, w, k, s, p = _mk(case, seed=31)
        g = torch.Generator().manual_seed(32)
        cout = w.shape[0]
        scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
        ref0 = F.conv3d(x, w, stride=s, padding=p)
        res = rb(torch.randn(ref0.shape, generator=g))
        ref = F.relu(ref0 * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1) + res)
        xa, wa = to_act(x, dev), to_w(w, dev)
        y, _ = ops.conv_fwd(xa, wa, k, s, p, scale=scale.to(dev), shift=shift.to(dev),
                            residual=to_act(res, dev), relu=True, splitk=True)
        assert_close(y, ref, TOL, case[0] + " split-K fused epilogue")
        y1, p1 = ops.conv_fwd(xa, wa, k, s, p, stats=True, splitk=True)
        y2, p2 = ops.conv_fwd(xa, wa, k, s, p, stats=True, splitk=True)
        assert torch.equal(y1, y2) and torch.equal(p1, p2)
        tot = p1.double().sum(0).cpu()
        assert torch.allclose(tot[0], ref0.double().sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=1e-2)
        y3, _ = ops.conv_fwd(xa, wa, k, s, p, tile=1)  # single-pass 64x128 kernel
        assert_close(y1, y3.float(), 8e-3, case[0] + " split-K vs single pass")


STRIDED = [
    # name, N, Cin, T, H, W, Cout, k, s, p
    ("s2_3x3_128", 2, 128, 2, 14, 14, 128, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("s2_3x3_odd", 1, 64, 3, 13, 11, 128, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("s2_1x1_256_512", 1, 256, 2, 14, 14, 512, (1, 1, 1), (1, 2, 2), (0, 0, 0)),
    ("s2_1x1_odd", 1, 64, 2, 9, 7, 128, (1, 1, 1), (1, 2, 2), (0, 0, 0)),
    ("s4_t7_fuse", 1, 32, 16, 5, 5, 64, (7, 1, 1), (4, 1, 1), (3, 0, 0)),
    ("s222_3x3x3", 1, 64, 6, 10, 10, 64, (3, 3, 3), (2, 2, 2), (1, 1, 1)),
]


@pytest.mark.parametrize("case", STRIDED, ids=[c[0] for c in STRIDED])
def test_strided_dgrad_stride_classes(case, dev):
    """dgrad of a strided conv tiles the input positions by stride class (each class walks only
    the taps that can reach it).  Checked against autograd, against the un-classed gather
    (VS_CONV_NOCLASS) and with the fused residual, on every tile config / staging variant."""
    from vidsitu_amd import ops

    x, w, k, s, p = _mk(case, seed=31)
    x.requires_grad_()
    y = F.conv3d(x, w, stride=s, padding=p)
    dy = rb(torch.randn(y.shape, generator=torch.Generator().manual_seed(32)))
    (dx_ref,) = torch.autograd.grad(y, x, dy)
    wt = ops.weight_transpose(to_w(w, dev))
    dya = to_act(dy, dev)
    r = rb(torch.randn(x.shape, generator=torch.Generator().manual_seed(33)))
    ra = to_act(r, dev)
    for tile in (None, 0, 1, 2, 3):
        for ring in (1, 2, 3):
            dx = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, tile=tile, ring=ring)
            assert_close(dx, dx_ref, TOL, f"{case[0]} tile {tile} ring {ring}")
            dxr = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, tile=tile, ring=ring, residual=ra)
            assert_close(dxr, dx_ref + r, TOL, f"{case[0]} tile {tile} ring {ring} +residual")
    old = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, noclass=True)
    assert_close(old, dx_ref, TOL, case[0] + " un-classed gather")


RING_CASES = [CASES[i] for i in (0, 1, 4, 5, 6, 9, 10, 11, 14, 15, 17)]


@pytest.mark.parametrize("ring", [2, 3, 4])
@pytest.mark.parametrize("case", RING_CASES, ids=[c[0] for c in RING_CASES])
def test_lds_dma_ring_is_bitwise_the_register_pipeline(case, ring, dev):
    """The LDS-DMA staging (buffer_load ... lds ring, VS_CONV_RING) feeds the same LDS image
    to the same MFMA order as the register-staged pipeline: identical bits, for the forward
    gather, the BN partials and both dgrad gathers, on every tile config that supports it."""
    from vidsitu_amd import ops

    x, w, k, s, p = _mk(case, seed=3)
    xa, wa = to_act(x, dev), to_w(w, dev)
    ref = F.conv3d(x, w, stride=s, padding=p)
    dy = rb(torch.randn(ref.shape, generator=torch.Generator().manual_seed(5)))
    dya, wt = to_act(dy, dev), ops.weight_transpose(wa)
    res = to_act(rb(torch.randn(x.shape, generator=torch.Generator().manual_seed(6))), dev)
    for tile in (0, 1, 2, 3, 4, 6, 7):
        y0, p0 = ops.conv_fwd(xa, wa, k, s, p, stats=True, tile=tile, ring=1)
        y1, p1 = ops.conv_fwd(xa, wa, k, s, p, stats=True, tile=tile, ring=ring)
        assert torch.equal(y0, y1) and torch.equal(p0, p1), f"{case[0]} fwd tile {tile} ring {ring}"
        d0 = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, residual=res, tile=tile, ring=1)
        d1 = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, residual=res, tile=tile, ring=ring)
        assert torch.equal(d0, d1), f"{case[0]} dgrad tile {tile} ring {ring}"
    assert_close(y1, ref, TOL, case[0] + " ring vs torch")


@pytest.mark.parametrize("ring", [2, 3])
@pytest.mark.parametrize("case", WG_CASES, ids=[c[0] for c in WG_CASES])
def test_wgrad_lds_dma_ring_is_bitwise_the_register_pipeline(case, ring, dev):
    """conv_wgrad_ring_kernel (LDS-DMA staging, tap-mask position table rebuilt a chunk ahead,
    pipeline never drained) accumulates the same tiles in the same order as conv_wgrad_kernel."""
    from vidsitu_amd import ops

    if case[7][0] * case[7][1] * case[7][2] > 31:
        pytest.skip("more than 31 taps: register-staged kernel only")
    x, w, k, s, p = _mk(case, seed=21)
    y = F.conv3d(x, w, stride=s, padding=p)
    dy = rb(torch.randn(y.shape, generator=torch.Generator().manual_seed(22)))
    xa, dya = to_act(x, dev), to_act(dy, dev)
    d0 = ops.conv_wgrad(dya, xa, k, s, p, ring=1)
    d1 = ops.conv_wgrad(dya, xa, k, s, p, ring=ring)
    assert torch.equal(d0, d1), f"{case[0]} ring {ring}: max diff {float((d0 - d1).abs().max()):.3e}"


def test_wgrad_ring_long_position_range(dev):
    """> 2 table chunks per block (the double-buffered position table wraps) and a ragged tail."""
    from vidsitu_amd import ops

    g = torch.Generator().manual_seed(5)
    x = rb(torch.randn(1, 128, 4, 40, 44, generator=g))      # 7040 positions, Cout x K' = one tile
    dy = rb(torch.randn(1, 128, 4, 40, 44, generator=g))
    k, s, p = (1, 3, 3), (1, 1, 1), (0, 1, 1)
    xa, dya = to_act(x, dev), to_act(dy, dev)
    d0 = ops.conv_wgrad(dya, xa, k, s, p, ring=1)
    for ring in (2, 3):
        assert torch.equal(d0, ops.conv_wgrad(dya, xa, k, s, p, ring=ring))
    xr = x.clone().requires_grad_()
    wr = torch.zeros(128, 128, 1, 3, 3, requires_grad=True)
    (gw,) = torch.autograd.grad(F.conv3d(xr, wr, padding=p), wr, dy)
    assert_close(d0, gw, TOL, "long-range wgrad vs autograd")


@pytest.mark.parametrize("n,t,hw", [(1, 32, 56), (8, 32, 56)], ids=["1clip_100352pos", "8clips_802816pos"])
@pytest.mark.parametrize("cin,cout,k,p", [(8, 8, (3, 1, 1), (1, 0, 0)), (8, 32, (1, 1, 1), (0, 0, 0)),
                                          (32, 8, (3, 1, 1), (1, 0, 0))], ids=["a_8_8_t3", "sc_8_32", "c_32_8_t3"])
@pytest.mark.parametrize("structured", [False, True], ids=["noise", "bn_like"])
def test_wgrad_vs_fp64_on_equal_bf16_operands_at_fast_res0_shapes(n, t, hw, cin, cout, k, p, structured, dev):
    """The tight bound behind tests/test_gpu_parity_full.py's loose one: at the full-resolution shapes of the fast
    pathway's first block (8 / 32 channels, 100 352 positions per clip) the layer-local comparison allows 1.5e-1 on two
    weight gradients, because those sums are cancellation-dominated (x >= 0 with a large mean against a dy that sums to
    ~0 per channel) and move 7-9 % with the operands' own bf16 roundings.  Here the kernel and an fp64 reference get the
    SAME bf16 operands: whatever is left is the kernel's own arithmetic (fp32 accumulation, fixed-order slab sum), which
    has to stay at the 1e-7 level -- a dropped term, a wrong tap or a mis-split position range is an O(1e-2 .. 1) error
    here.  `structured` builds operands with the real ones' structure.  (was tools/probes/wgrad_bigP.py, round 3:
    1.4e-7 .. 6.7e-7)"""
    from vidsitu_amd import ops

    g = torch.Generator().manual_seed(n * 1000 + cin * 10 + cout + int(structured))
    x = torch.randn(n, cin, t, hw, hw, generator=g)
    dy = torch.randn(n, cout, t, hw, hw, generator=g)
    if structured:
        x = x.abs() + 1.0
        dy = dy - dy.mean(dim=(0, 2, 3, 4), keepdim=True)
    x, dy = rb(x), rb(dy)
    # fp64 reference on the GPU (torch's own fp64 convolution backward; no MFMA, no bf16)
    xd, dyd = x.to(dev).double(), dy.to(dev).double()
    w = torch.zeros(cout, cin, *k, dtype=torch.float64, device=dev, requires_grad=True)
    ref = torch.autograd.grad(F.conv3d(xd, w, padding=p), w, dyd)[0]
    got = ops.conv_wgrad(to_act(dy, dev), to_act(x, dev), k, (1, 1, 1), p).double()
    err = float((got - ref).norm() / ref.norm())
    print(f"n{n} cin{cin} cout{cout} k{k} structured={structured}: rel_l2 vs fp64 {err:.3e}")
    assert err <= 5e-6, err


def test_wgrad_is_bitwise_reproducible(dev):
    from vidsitu_amd import ops

    x, w, k, s, p = _mk(CASES[6], seed=2)
    dy = rb(torch.randn(F.conv3d(x, w, stride=s, padding=p).shape))
    a = ops.conv_wgrad(to_act(dy, dev), to_act(x, dev), k, s, p)
    b = ops.conv_wgrad(to_act(dy, dev), to_act(x, dev), k, s, p)
    assert torch.equal(a, b)


def test_pack_input_layout(dev):
    from vidsitu_amd import ops

    x = torch.randn(2, 3, 4, 6, 10)
    y = ops.pack_input(x.to(dev))
    assert tuple(y.shape) == (2, 8, 4, 6, 10)
    assert torch.equal(y[:, :3].float().cpu(), rb(x))
    assert float(y[:, 3:].float().abs().max()) == 0.0
    y2 = ops.pack_input(x.to(dev).to(torch.bfloat16))
    assert torch.equal(y2.float(), y.float())
    # stem layout (4 channels per pixel): the 8-pixels-per-thread kernel (T*H*W % 8 == 0) and the
    # one-pixel fallback, fp32 and bf16 inputs
    for shape in [(2, 3, 4, 6, 12), (1, 3, 3, 5, 7), (3, 2, 2, 8, 8)]:
        xs = torch.randn(*shape)
        for inp in (xs.to(dev), xs.to(dev).to(torch.bfloat16)):
            y4 = ops.pack_input(inp, 4)
            assert tuple(y4.shape) == (shape[0], 4) + shape[2:]
            assert torch.equal(y4[:, :shape[1]].float().cpu(), rb(xs)), shape
            assert float(y4[:, shape[1]:].float().abs().max()) == 0.0


@pytest.mark.parametrize("cout,kt,t,h,w", [(64, 1, 2, 32, 32), (8, 5, 6, 32, 32), (64, 1, 1, 36, 44),
                                           (8, 5, 3, 20, 52), (32, 3, 4, 64, 64),
                                           # <= 8 channels: two output frames per pass (stem_pair_kernel): frame
                                           # chunks of 8, odd frame counts, one frame, 3 temporal taps, tile tails
                                           (8, 5, 17, 40, 44), (8, 5, 1, 32, 32), (8, 3, 9, 24, 70),
                                           (8, 5, 32, 64, 64)])
def test_stem_kernel_matches_torch(cout, kt, t, h, w, dev):
    """Dedicated Cin=3 stem kernel (conv_stem.hip): patch-in-LDS implicit GEMM, incl. tile tails,
    temporal padding, fused affine+ReLU and the BN partials."""
    from vidsitu_amd import ops

    g = torch.Generator().manual_seed(cout + kt)
    x = rb(torch.randn(2, 3, t, h, w, generator=g))
    wt = rb(torch.randn(cout, 3, kt, 7, 7, generator=g) / (147 * kt) ** 0.5)
    ref = F.conv3d(x, wt, stride=(1, 2, 2), padding=(kt // 2, 3, 3))
    x4 = ops.pack_input(x.to(dev), 4)
    assert tuple(x4.shape) == (2, 4, t, h, w)
    wp = ops.pack_stem_weight(wt.to(dev))
    y, partials = ops.stem_conv_fwd(x4, wp, cout, kt, stats=True)
    assert tuple(y.shape) == tuple(ref.shape)
    assert_close(y, ref, TOL, "stem conv")
    tot = partials.double().sum(0).cpu()
    assert torch.allclose(tot[0], ref.double().sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=1e-2)
    assert torch.allclose(tot[1], (ref.double() ** 2).sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=1e-2)
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    y2, _ = ops.stem_conv_fwd(x4, wp, cout, kt, scale=scale.to(dev), shift=shift.to(dev), relu=True)
    assert_close(y2, F.relu(ref * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)), TOL,
                 "stem conv + affine + relu")


@pytest.mark.parametrize("cout,kt,t,h,w", [(64, 1, 2, 32, 32), (8, 5, 6, 32, 32), (64, 1, 1, 36, 44),
                                           (8, 5, 5, 20, 52), (16, 3, 4, 32, 48),
                                           # <= 8 channels: two output frames per pass (stem_wgrad_pair_kernel)
                                           (8, 5, 17, 40, 44), (8, 5, 1, 32, 32), (8, 3, 9, 24, 70),
                                           (8, 5, 32, 64, 64)])
def test_stem_wgrad_matches_autograd(cout, kt, t, h, w, dev):
    from vidsitu_amd import ops

    g = torch.Generator().manual_seed(cout * 3 + kt)
    x = rb(torch.randn(2, 3, t, h, w, generator=g))
    wt = rb(torch.randn(cout, 3, kt, 7, 7, generator=g) / (147 * kt) ** 0.5).requires_grad_()
    y = F.conv3d(x, wt, stride=(1, 2, 2), padding=(kt // 2, 3, 3))
    dy = rb(torch.randn(y.shape, generator=g))
    (dw_ref,) = torch.autograd.grad(y, wt, dy)
    dw = ops.stem_conv_wgrad(to_act(dy, dev), ops.pack_input(x.to(dev), 4), kt)
    assert tuple(dw.shape) == tuple(dw_ref.shape)
    assert_close(dw, dw_ref, 5e-3, "stem wgrad")
    dw2 = ops.stem_conv_wgrad(to_act(dy, dev), ops.pack_input(x.to(dev), 4), kt)
    assert torch.equal(dw.contiguous(), dw2.contiguous())  # fixed-order slab reduce


def test_tiled_batched_transposes_equal_the_per_element_kernels(dev):
    """`vs_weight_transpose_tiled` (LDS tiles, one launch for all weights) against the per-element batched
    kernels: conv weights [Cout][taps][Cin] bf16 and linear weights [N][K] fp32, ragged shapes."""
    from vidsitu_amd import ops

    g = torch.Generator().manual_seed(0)
    for dtype, shapes in ((torch.bfloat16, [(64, 27, 8), (8, 35, 3), (256, 1, 64), (80, 9, 72), (512, 3, 128), (33, 5, 17)]),
                          (torch.float32, [(1024, 1, 2304), (1564, 1, 1152), (100, 1, 33), (64, 1, 64), (7, 1, 300)])):
        rows, off, first = [], 0, 0
        for cout, taps, cin in shapes:
            n = cout * taps * cin
            rows.append([off, cout, taps, cin, first])
            off += (n + 3) // 4 * 4
            first += n
        table = torch.tensor(rows, dtype=torch.int64, device=dev)
        src = torch.randn(off, generator=g).to(dtype).to(dev)
        a, b = torch.zeros_like(src), torch.zeros_like(src)
        fn = ops.weight_transpose_batched if dtype == torch.bfloat16 else ops.transpose_f32_batched
        fn(src, a, table, first, tiled=False)
        fn(src, b, table, first, tiled=True)
        assert torch.equal(a.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                           b.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
        for (o, cout, taps, cin, _) in rows:  # and against torch
            n = cout * taps * cin
            want = src[o:o + n].view(cout, taps, cin).permute(2, 1, 0).contiguous().view(-1)
            assert torch.equal(b[o:o + n], want)


BNS_CASES = [CASES[i] for i in (0, 1, 4, 5, 6, 7, 9, 10, 11, 14, 15)] + STRIDED[:4] + [STRIDED[5]]


@pytest.mark.parametrize("case", BNS_CASES, ids=[c[0] for c in BNS_CASES])
def test_dgrad_emits_the_producer_bn_backward_sums(case, dev, guarded_partials):
    """vs_conv_dgrad_bnstats: dx bitwise the plain dgrad, and the per-tile partial sums add up to what
    vs_bn_bwd_reduce (recomputed-mask mode) computes from that dx and the producer's saved conv output --
    pointwise / gathered / strided dgrads (stride classes incl. classes no tap reaches), every tile shape
    the path is built for, register pipeline and LDS-DMA ring."""
    from vidsitu_amd import ops
    import ctypes as C

    x, w, k, s, p = _mk(case, seed=41)
    cin = x.shape[1]
    y = F.conv3d(x, w, stride=s, padding=p)
    dy = rb(torch.randn(y.shape, generator=torch.Generator().manual_seed(42)))
    wt = ops.weight_transpose(to_w(w, dev))
    dya = to_act(dy, dev)
    g = torch.Generator().manual_seed(43)
    bn_y = to_act(rb(torch.randn(x.shape, generator=g)), dev)  # the producer's saved conv output
    mean = (torch.randn(cin, generator=g) * 0.2).to(dev)
    invstd = (torch.rand(cin, generator=g) + 0.5).to(dev)
    gamma = (torch.randn(cin, generator=g)).to(dev)
    beta = (torch.randn(cin, generator=g) * 0.3).to(dev)
    plain = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p)
    rows, c = ops.act_rows(plain), cin
    nblk = ops._lib.load().vs_bn_bwd_reduce_rows(rows, c)
    if nblk > 0:
        want = torch.empty((nblk, 2, c), dtype=torch.float32, device=dev)
        ops._lib.call("vs_bn_bwd_reduce", ops._ptr(plain), None, ops._ptr(bn_y), ops._ptr(mean), ops._ptr(invstd),
                      ops._ptr(gamma), ops._ptr(beta), ops._ptr(want), rows, c, ops.act_ld(plain), 0,
                      ops.act_ld(bn_y), 1, ops._stream())
        want, tol = want.double().sum(0).cpu(), 1e-5
    else:  # the reduce kernel wants C/8 a power of two: torch restatement (mask ties may round differently)
        v = lambda t: t.view(1, -1, 1, 1, 1)
        xh = (bn_y.float() - v(mean)) * v(invstd)
        gm = torch.where(xh * v(gamma) + v(beta) > 0, plain.float(), torch.zeros((), device=dev))
        want = torch.stack([gm.double().sum((0, 2, 3, 4)), (gm * xh).double().sum((0, 2, 3, 4))]).cpu()
        tol = 2e-3
    scale = float(want.abs().max())
    tried = 0
    for tile in (None, 0, 1, 3):
        for ring in (1, 2, 3):
            dx, part = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, tile=tile, ring=ring,
                                      bn_stats=(bn_y, mean, invstd, gamma, beta))
            if part is None:
                continue
            tried += 1
            ref = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, tile=tile, ring=ring)
            assert torch.equal(dx.view(torch.int16), ref.view(torch.int16)), (case[0], tile, ring)
            got = part.double().sum(0).cpu()
            err = float((got - want).abs().max()) / scale
            assert err < tol, (case[0], tile, ring, err)
    assert tried >= 3, "no tile configuration took the fused path"
    # residual input (the gradient over the identity branch) + the unit's ReLU mask as bits: the pairing of
    # the previous block's c unit.  A recomputed mask with a residual is not built: (dx, None).
    r = to_act(rb(torch.randn(x.shape, generator=g)), dev)
    _, none = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, residual=r, bn_stats=(bn_y, mean, invstd, gamma, beta))
    assert none is None
    bits = torch.randint(0, 256, (rows, c // 8), generator=g, dtype=torch.uint8).to(dev)

    def sums_from(dz):  # what the reduce pass computes from this dz (bit-mask mode)
        if nblk > 0:
            w_ = torch.empty((nblk, 2, c), dtype=torch.float32, device=dev)
            ops._lib.call("vs_bn_bwd_reduce", ops._ptr(dz), ops._ptr(bits), ops._ptr(bn_y), ops._ptr(mean),
                          ops._ptr(invstd), None, None, ops._ptr(w_), rows, c, ops.act_ld(dz), c // 8,
                          ops.act_ld(bn_y), 2, ops._stream())
            return w_.double().sum(0).cpu()
        v = lambda t: t.view(1, -1, 1, 1, 1)
        xh = (bn_y.float() - v(mean)) * v(invstd)
        keep = ((bits.view(rows, c // 8, 1) >> torch.arange(8, device=dev, dtype=torch.uint8)) & 1).bool()
        keep = keep.view(x.shape[0], *x.shape[2:], c).permute(0, 4, 1, 2, 3)
        gm = torch.where(keep, dz.float(), torch.zeros((), device=dev))
        return torch.stack([gm.double().sum((0, 2, 3, 4)), (gm * xh).double().sum((0, 2, 3, 4))]).cpu()

    strided = any(v != 1 for v in s)
    tried = 0
    for tile in (None, 0, 1, 3):
        for ring in (1, 2, 3):
            dx, part = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, tile=tile, ring=ring, residual=r,
                                      bn_stats=(bn_y, mean, invstd, None, None, bits))
            if part is None:
                continue
            tried += 1
            ref = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, tile=tile, ring=ring, residual=r)
            assert torch.equal(dx.view(torch.int16), ref.view(torch.int16)), (case[0], tile, ring)
            want = sums_from(ref)
            err = float((part.double().sum(0).cpu() - want).abs().max()) / float(want.abs().max())
            assert err < 1e-5, (case[0], tile, ring, "residual", err)
    assert tried == 0 if strided else tried >= 3  # a strided dgrad with a residual is not fused


def _unpack_bits(bits, shape):
    """uint8 [rows, C/8] -> bool mask of logical shape [N, C, T, H, W]."""
    n, c, t, h, w = shape
    rows = n * t * h * w
    keep = ((bits.view(rows, c // 8, 1) >> torch.arange(8, device=bits.device, dtype=torch.uint8)) & 1).bool()
    return keep.view(n, t, h, w, c).permute(0, 4, 1, 2, 3)


MR_CASES = [CASES[i] for i in (0, 1, 4, 5, 9, 10, 14, 17)] + STRIDED[:5]


@pytest.mark.parametrize("case", MR_CASES, ids=[c[0] for c in MR_CASES])
def test_dgrad_masked_residual_and_inplace_accumulate(case, dev):
    """vs_conv_dgrad_ex: (1) `residual_bits` -- the residual is an unmasked gradient and the epilogue applies the
    unit's ReLU bit mask to it: bitwise the plain dgrad fed the pre-masked residual, on every tile / staging
    variant, the small-channel direct kernel included, and together with the BN-backward-sums epilogue;
    (2) `inplace` -- out aliases the residual (an accumulating dgrad): bitwise the out-of-place result,
    including strided dgrads whose zero-tap stride classes are skipped."""
    from vidsitu_amd import ops

    x, w, k, s, p = _mk(case, seed=51)
    cin = x.shape[1]
    y = F.conv3d(x, w, stride=s, padding=p)
    g = torch.Generator().manual_seed(52)
    dya = to_act(rb(torch.randn(y.shape, generator=g)), dev)
    wt = ops.weight_transpose(to_w(w, dev))
    r = to_act(rb(torch.randn(x.shape, generator=g)), dev)
    xs = tuple(x.shape)
    rows = ops.act_rows(r)
    bits = torch.randint(0, 256, (rows, cin // 8), generator=g, dtype=torch.uint8).to(dev)
    keep = _unpack_bits(bits, xs)
    r_masked = ops.new_act(*xs, device=dev)
    r_masked.copy_(torch.where(keep, r, torch.zeros((), device=dev, dtype=r.dtype)))
    for tile in (None, 0, 1, 3):
        for ring in (1, 2, 3):
            want = ops.conv_dgrad(dya, wt, xs, k, s, p, tile=tile, ring=ring, residual=r_masked)
            got = ops.conv_dgrad(dya, wt, xs, k, s, p, tile=tile, ring=ring, residual=r, residual_bits=bits)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (case[0], tile, ring, "mask")
            plain = ops.conv_dgrad(dya, wt, xs, k, s, p, tile=tile, ring=ring, residual=r)
            acc = ops.new_act(*xs, device=dev)
            acc.copy_(r)
            out = ops.conv_dgrad(dya, wt, xs, k, s, p, tile=tile, ring=ring, residual=acc, inplace=True)
            assert out.data_ptr() == acc.data_ptr()
            assert torch.equal(out.view(torch.int16), plain.view(torch.int16)), (case[0], tile, ring, "inplace")
    # with the producer's BN-backward sums in the same epilogue (unit-stride only: see vs_conv_dgrad_bnstats_rows)
    bn_y = to_act(rb(torch.randn(x.shape, generator=g)), dev)
    mean = (torch.randn(cin, generator=g) * 0.2).to(dev)
    invstd = (torch.rand(cin, generator=g) + 0.5).to(dev)
    pbits = torch.randint(0, 256, (rows, cin // 8), generator=g, dtype=torch.uint8).to(dev)
    dx1, p1 = ops.conv_dgrad(dya, wt, xs, k, s, p, residual=r_masked, bn_stats=(bn_y, mean, invstd, None, None, pbits))
    dx2, p2 = ops.conv_dgrad(dya, wt, xs, k, s, p, residual=r, residual_bits=bits,
                             bn_stats=(bn_y, mean, invstd, None, None, pbits))
    assert torch.equal(dx1.view(torch.int16), dx2.view(torch.int16))
    assert (p1 is None) == (p2 is None)
    if p1 is not None:
        assert torch.equal(p1, p2)


def test_direct_kernel_masked_residual(dev):
    """The register-resident small-channel kernel (N <= 32 columns) applies residual_bits as well."""
    from vidsitu_amd import ops

    g = torch.Generator().manual_seed(61)
    n, cin, t, h, w, cout, k, s, p = 2, 32, 4, 12, 12, 8, (1, 3, 3), (1, 1, 1), (0, 1, 1)
    wgt = rb(torch.randn(cout, cin, *k, generator=g) * 0.1)
    dya = to_act(rb(torch.randn(n, cout, t, h, w, generator=g)), dev)
    wt = ops.weight_transpose(to_w(wgt, dev))
    xs = (n, cin, t, h, w)
    r = to_act(rb(torch.randn(xs, generator=g)), dev)
    bits = torch.randint(0, 256, (n * t * h * w, cin // 8), generator=g, dtype=torch.uint8).to(dev)
    r_masked = ops.new_act(*xs, device=dev)
    r_masked.copy_(torch.where(_unpack_bits(bits, xs), r, torch.zeros((), device=dev, dtype=r.dtype)))
    import ctypes as C
    d = ops.make_desc(xs, cin, dya.shape, cout, k, s, p, 0)
    out = (C.c_int * 5)()
    ops._lib.load().vs_conv_plan(C.byref(d), 1, out)
    assert out[4] == 1, "expected the direct kernel for this shape"
    want = ops.conv_dgrad(dya, wt, xs, k, s, p, residual=r_masked)
    got = ops.conv_dgrad(dya, wt, xs, k, s, p, residual=r, residual_bits=bits)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


# name, N, Cin, T, H, W, Cout, k, p   (unit stride, "same" padding): shapes the halo-image kernel takes
HALO_CASES = [
    ("s4b_3x3_256", 2, 256, 8, 14, 14, 256, (1, 3, 3), (0, 1, 1)),
    ("s4a_t3_1024_256", 2, 1024, 8, 14, 14, 256, (3, 1, 1), (1, 0, 0)),
    ("s5b_3x3_512", 8, 512, 8, 7, 7, 512, (1, 3, 3), (0, 1, 1)),
    ("s5a_t3_1024_512", 8, 1024, 8, 7, 7, 512, (3, 1, 1), (1, 0, 0)),
    ("s3b_3x3_128", 1, 128, 8, 28, 28, 128, (1, 3, 3), (0, 1, 1)),
    ("s2b_3x3_64", 1, 64, 4, 56, 56, 64, (1, 3, 3), (0, 1, 1)),
    ("odd_3x3_64_72", 4, 64, 5, 13, 11, 72, (1, 3, 3), (0, 1, 1)),
    ("odd_t3_128_64", 12, 128, 6, 5, 7, 64, (3, 1, 1), (1, 0, 0)),
    ("t5_64_64", 4, 64, 8, 9, 9, 64, (5, 1, 1), (2, 0, 0)),
    ("5x5_64_64", 2, 64, 4, 20, 20, 64, (1, 5, 5), (0, 2, 2)),
    ("3x1_64_136", 2, 64, 4, 20, 20, 136, (1, 3, 1), (0, 1, 0)),
    ("fast_t32_3x3", 2, 64, 32, 7, 7, 64, (1, 3, 3), (0, 1, 1)),
    # 128-column tiles (never chosen at 8 clips per GPU; 16+ clips of slow s5 are): 224 / 128 rows, forward / dgrad
    ("w128_3x3_224", 2, 64, 8, 28, 20, 512, (1, 3, 3), (0, 1, 1)),
    ("w128_t3_224", 2, 64, 8, 28, 28, 512, (3, 1, 1), (1, 0, 0)),
    ("w128_t3_128", 4, 64, 8, 9, 28, 512, (3, 1, 1), (1, 0, 0)),
    ("w128_3x3_128", 4, 64, 8, 12, 20, 512, (1, 3, 3), (0, 1, 1)),
    ("w128_dgrad_t3", 16, 128, 8, 9, 28, 128, (3, 1, 1), (1, 0, 0)),
    ("w128_dgrad_3x3", 16, 128, 8, 12, 20, 128, (1, 3, 3), (0, 1, 1)),
    ("s5b_3x3_512_n32", 32, 512, 8, 7, 7, 512, (1, 3, 3), (0, 1, 1)),
]
_HALO_W128 = {"w128_3x3_224": (0, 224), "w128_t3_224": (0, 224), "w128_t3_128": (0, 128), "w128_3x3_128": (0, 128),
              "w128_dgrad_t3": (1, 128), "w128_dgrad_3x3": (1, 128), "s5b_3x3_512_n32": (0, 224)}


def _plan(ops, xs, ys, x_ld, y_ld, k, s, p, dgrad, flags=_lib.VS_CONV_FORCEHALO):
    import ctypes as C
    d = ops.make_desc(xs, x_ld, ys, y_ld, k, s, p, flags)
    out = (C.c_int * 5)()
    ops._lib.load().vs_conv_plan(C.byref(d), dgrad, out)
    return list(out)


@pytest.mark.parametrize("case", HALO_CASES, ids=[c[0] for c in HALO_CASES])
def test_halo_image_kernel_fwd_and_dgrad(case, dev, guarded_partials):
    """conv_halo.hip (unit-stride [kT,1,1] / [1,kH,kW] convs, the activation patch incl. its halo staged once
    per 64-channel chunk): forward with every epilogue (BN-stat partials, affine + ReLU, residual) and the data
    gradient (plain, + residual, + masked residual, + the producer's BN-backward sums) against torch and
    against the implicit-GEMM kernel (VS_CONV_NOHALO) -- ragged line / spatial groups, 3, 5, 9 and 25 taps."""
    from vidsitu_amd import ops

    name, n, cin, t, h, w, cout, k, p = case
    s = (1, 1, 1)
    g = torch.Generator().manual_seed(71)
    x = rb(torch.randn(n, cin, t, h, w, generator=g))
    wgt = rb(torch.randn(cout, cin, *k, generator=g) / (cin * k[0] * k[1] * k[2]) ** 0.5)
    xa, wa = to_act(x, dev), to_w(wgt, dev)
    ys = (n, cout, t, h, w)
    assert _plan(ops, tuple(x.shape), ys, cin, cout, k, s, p, 0)[4] == 2, "forward did not take the halo kernel"
    # (the data gradient reduces over Cout in 64-channel chunks: 72 / 136 output channels stay on the other kernel)
    assert (_plan(ops, tuple(x.shape), ys, cin, cout, k, s, p, 1)[4] == 2) == (cout % 64 == 0), "dgrad kernel choice"
    if name in _HALO_W128:  # the case exists for the 128-column variant: make sure that is what runs
        dg, bm = _HALO_W128[name]
        assert _plan(ops, tuple(x.shape), ys, cin, cout, k, s, p, dg)[:2] == [bm, 128], "not the 128-column tile"
    ref = F.conv3d(x, wgt, stride=s, padding=p)
    # forward: raw + BN-stat partials
    y, part = ops.conv_fwd(xa, wa, k, s, p, stats=True, halo="force")
    assert_close(y, ref, TOL, name + " fwd")
    y0, part0 = ops.conv_fwd(xa, wa, k, s, p, stats=True, halo=False)
    assert_close(y, y0.float(), 4e-3, name + " fwd vs implicit GEMM")
    tot, tot0 = part.double().sum(0).cpu(), part0.double().sum(0).cpu()
    assert torch.allclose(tot, tot0, rtol=2e-3, atol=2e-3 * float(tot0.abs().max()))
    assert torch.allclose(tot[0], ref.double().sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=2e-2)
    # forward: folded BN + residual + ReLU into a wider (concat) buffer
    sc = (torch.rand(cout, generator=g) + 0.5).to(dev)
    sh = torch.randn(cout, generator=g).to(dev)
    r = rb(torch.randn(ref.shape, generator=g))
    buf = ops.new_act(n, cout + 16, t, h, w, dev, zero=True)
    out = ops.channel_slice(buf, 8, cout)
    ops.conv_fwd(xa, wa, k, s, p, out=out, scale=sc, shift=sh, residual=to_act(r, dev), relu=True, halo="force")
    want = (ref * sc.cpu().view(1, -1, 1, 1, 1) + sh.cpu().view(1, -1, 1, 1, 1) + r).relu()
    assert_close(out, want, TOL, name + " fwd epilogue")
    assert float(buf[:, :8].abs().max()) == 0.0 and float(buf[:, 8 + cout:].abs().max()) == 0.0
    # data gradient
    xg = x.clone().requires_grad_()
    yy = F.conv3d(xg, wgt, stride=s, padding=p)
    dy = rb(torch.randn(yy.shape, generator=g))
    (dx_ref,) = torch.autograd.grad(yy, xg, dy)
    wt = ops.weight_transpose(wa)
    dya = to_act(dy, dev)
    dx = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, halo="force")
    assert_close(dx, dx_ref, TOL, name + " dgrad")
    # two fp32 accumulation orders rounded to bf16: one bf16 ulp of the largest output is 2^-8 .. 2^-7 of it
    assert_close(dx, ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, halo=False).float(), 2.0 ** -7,
                 name + " dgrad vs implicit GEMM")
    rr = rb(torch.randn(x.shape, generator=g))
    rra = to_act(rr, dev)
    dxr = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, residual=rra, halo="force")
    assert_close(dxr, dx_ref + rr, TOL, name + " dgrad + residual")
    rows = ops.act_rows(rra)
    bits = torch.randint(0, 256, (rows, cin // 8), generator=g, dtype=torch.uint8).to(dev)
    keep = _unpack_bits(bits, tuple(x.shape))
    dxm = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, residual=rra, residual_bits=bits, halo="force")
    assert_close(dxm, dx_ref + torch.where(keep.cpu(), rr, torch.zeros(())), TOL, name + " dgrad + masked residual")
    # + the BN-backward sums of the unit this dx belongs to: dx bitwise the plain launch, sums = the reduce pass
    bn_y = to_act(rb(torch.randn(x.shape, generator=g)), dev)
    mean = (torch.randn(cin, generator=g) * 0.2).to(dev)
    invstd = (torch.rand(cin, generator=g) + 0.5).to(dev)
    gamma, beta = torch.randn(cin, generator=g).to(dev), (torch.randn(cin, generator=g) * 0.3).to(dev)
    dxs, psum = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, bn_stats=(bn_y, mean, invstd, gamma, beta), halo="force")
    assert psum is not None and torch.equal(dxs.view(torch.int16), dx.view(torch.int16))
    v = lambda a: a.view(1, -1, 1, 1, 1)
    xh = (bn_y.float() - v(mean)) * v(invstd)
    gm = torch.where(xh * v(gamma) + v(beta) > 0, dx.float(), torch.zeros((), device=dev))
    want = torch.stack([gm.double().sum((0, 2, 3, 4)), (gm * xh).double().sum((0, 2, 3, 4))]).cpu()
    got = psum.double().sum(0).cpu()
    assert float((got - want).abs().max()) / float(want.abs().max()) < 2e-3
    dxb, psb = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, residual=rra, bn_stats=(bn_y, mean, invstd, None, None, bits),
                                halo="force")
    assert psb is not None and torch.equal(dxb.view(torch.int16), dxr.view(torch.int16))
    gm = torch.where(keep, dxr.float(), torch.zeros((), device=dev))
    want = torch.stack([gm.double().sum((0, 2, 3, 4)), (gm * xh).double().sum((0, 2, 3, 4))]).cpu()
    assert float((psb.double().sum(0).cpu() - want).abs().max()) / float(want.abs().max()) < 1e-5


# name, N, Cin, T, H, W, Cout, k, s, p: few-tile, deep-K shapes for the in-launch split-K plan of the 128 x 128 tile
SPLITK_IL_CASES = [
    ("s5a_t3_1024_512", 2, 1024, 4, 7, 7, 512, (3, 1, 1), (1, 1, 1), (1, 0, 0)),      # 4 x 4 tiles, 48 k-steps
    ("s5b_3x3_512", 2, 512, 4, 7, 7, 512, (1, 3, 3), (1, 1, 1), (0, 1, 1)),           # 72 k-steps
    ("pw_2048_512", 2, 2048, 2, 7, 7, 512, (1, 1, 1), (1, 1, 1), (0, 0, 0)),          # pointwise dense, 32 k-steps
    ("3x3_strided_256_256", 2, 256, 4, 14, 14, 256, (1, 3, 3), (1, 2, 2), (0, 1, 1)),  # its dgrad: stride classes
    ("ragged_136_264", 3, 136, 3, 13, 11, 264, (1, 3, 3), (1, 1, 1), (0, 1, 1)),      # K = 1224 (tail), N = 256 + 8, M = 1287
    ("short_k_512_128", 2, 512, 2, 7, 7, 128, (1, 1, 1), (1, 1, 1), (0, 0, 0)),       # 8 k-steps: S = 2
]


@pytest.mark.parametrize("case", SPLITK_IL_CASES, ids=[c[0] for c in SPLITK_IL_CASES])
def test_in_launch_splitk_fwd_and_dgrad(case, dev, guarded_partials):
    """In-launch split-K of the 128 x 128 tile kernel (S blocks per tile store their partial accumulators, the tile's
    last arriver sums them in split order and runs the fused epilogue): forward with every epilogue and the data
    gradient (plain, + residual, + masked residual, + BN-backward sums; strided: stride classes) against torch and
    against the unsplit launch; 30 repeats bit for bit (the sum must not depend on which block arrives last); the
    arrival counters are back at zero after every launch."""
    from vidsitu_amd import ops

    name, n, cin, t, h, w, cout, k, s, p = case
    g = torch.Generator().manual_seed(89)
    x = rb(torch.randn(n, cin, t, h, w, generator=g))
    wgt = rb(torch.randn(cout, cin, *k, generator=g) / (cin * k[0] * k[1] * k[2]) ** 0.5)
    xa, wa = to_act(x, dev), to_w(wgt, dev)
    ref = F.conv3d(x, wgt, stride=s, padding=p)
    ys = tuple(ref.shape)
    IL = _lib.VS_CONV_SPLITK_IL  # (+ NOHALO | NOPW | NODEEP: the tile kernel)
    other = _lib.VS_CONV_NOHALO | _lib.VS_CONV_NOPW | _lib.VS_CONV_NODEEP
    pl = _plan(ops, tuple(x.shape), ys, cin, cout, k, s, p, 0, IL | other)
    assert pl[4] == 5 and pl[3] >= 2 and pl[0] == 128 and pl[1] == 128, f"forward did not take the in-launch split: {list(pl)}"
    kw = dict(halo=False, pw=False, deep=False)
    y, part = ops.conv_fwd(xa, wa, k, s, p, stats=True, splitk_il=True, **kw)
    assert_close(y, ref, TOL, name + " fwd")
    y0, part0 = ops.conv_fwd(xa, wa, k, s, p, stats=True, splitk_il=False, tile=0, ring=2, **kw)
    assert_close(y, y0.float(), 4e-3, name + " fwd vs unsplit")
    assert part.shape == part0.shape
    tot, tot0 = part.double().sum(0).cpu(), part0.double().sum(0).cpu()
    assert torch.allclose(tot, tot0, rtol=2e-3, atol=2e-3 * float(tot0.abs().max()))
    for _ in range(30):  # run to run: bit for bit, whoever arrives last
        y2, part2 = ops.conv_fwd(xa, wa, k, s, p, stats=True, splitk_il=True, **kw)
        assert torch.equal(y2.view(torch.int16), y.view(torch.int16)) and torch.equal(part2, part)
    ws = ops._workspace(1, dev, "splitk")
    assert int(ws[:4096].view(torch.int32).abs().max()) == 0, "arrival counters not cleared"
    sc = (torch.rand(cout, generator=g) + 0.5).to(dev)
    sh = torch.randn(cout, generator=g).to(dev)
    r = rb(torch.randn(ref.shape, generator=g))
    buf = ops.new_act(ys[0], cout + 16, *ys[2:], dev, zero=True)
    out = ops.channel_slice(buf, 8, cout)
    ops.conv_fwd(xa, wa, k, s, p, out=out, scale=sc, shift=sh, residual=to_act(r, dev), relu=True, splitk_il=True, **kw)
    want = (ref * sc.cpu().view(1, -1, 1, 1, 1) + sh.cpu().view(1, -1, 1, 1, 1) + r).relu()
    assert_close(out, want, TOL, name + " fwd epilogue")
    assert float(buf[:, :8].abs().max()) == 0.0 and float(buf[:, 8 + cout:].abs().max()) == 0.0
    if cout * k[0] * k[1] * k[2] < 512:
        return  # the data gradient's reduction is shorter than 8 k-steps: nothing to split
    xg = x.clone().requires_grad_()
    yy = F.conv3d(xg, wgt, stride=s, padding=p)
    dy = rb(torch.randn(yy.shape, generator=g))
    (dx_ref,) = torch.autograd.grad(yy, xg, dy)
    wt = ops.weight_transpose(wa)
    dya = to_act(dy, dev)
    xs = tuple(x.shape)
    pld = _plan(ops, xs, ys, cin, cout, k, s, p, 1, IL | other)
    assert pld[4] == 5 and pld[3] >= 2, f"dgrad did not take the in-launch split: {list(pld)}"
    dx = ops.conv_dgrad(dya, wt, xs, k, s, p, splitk_il=True, **kw)
    assert_close(dx, dx_ref, TOL, name + " dgrad")
    assert_close(dx, ops.conv_dgrad(dya, wt, xs, k, s, p, splitk_il=False, **kw).float(), 2.0 ** -7, name + " dgrad vs unsplit")
    for _ in range(10):
        assert torch.equal(ops.conv_dgrad(dya, wt, xs, k, s, p, splitk_il=True, **kw).view(torch.int16), dx.view(torch.int16))
    rr = rb(torch.randn(x.shape, generator=g))
    rra = to_act(rr, dev)
    dxr = ops.conv_dgrad(dya, wt, xs, k, s, p, residual=rra, splitk_il=True, **kw)
    assert_close(dxr, dx_ref + rr, TOL, name + " dgrad + residual")
    rows = ops.act_rows(rra)
    bits = torch.randint(0, 256, (rows, cin // 8), generator=g, dtype=torch.uint8).to(dev)
    keep = _unpack_bits(bits, xs)
    dxm = ops.conv_dgrad(dya, wt, xs, k, s, p, residual=rra, residual_bits=bits, splitk_il=True, **kw)
    assert_close(dxm, dx_ref + torch.where(keep.cpu(), rr, torch.zeros(())), TOL, name + " dgrad + masked residual")
    bn_y = to_act(rb(torch.randn(x.shape, generator=g)), dev)
    mean = (torch.randn(cin, generator=g) * 0.2).to(dev)
    invstd = (torch.rand(cin, generator=g) + 0.5).to(dev)
    gamma, beta = torch.randn(cin, generator=g).to(dev), (torch.randn(cin, generator=g) * 0.3).to(dev)
    dxs, psum = ops.conv_dgrad(dya, wt, xs, k, s, p, bn_stats=(bn_y, mean, invstd, gamma, beta), splitk_il=True, **kw)
    assert psum is not None, "the in-launch split keeps the fused BN-backward sums"
    assert torch.equal(dxs.view(torch.int16), dx.view(torch.int16))
    v = lambda a: a.view(1, -1, 1, 1, 1)
    xh = (bn_y.float() - v(mean)) * v(invstd)
    gm = torch.where(xh * v(gamma) + v(beta) > 0, dx.float(), torch.zeros((), device=dev))
    want = torch.stack([gm.double().sum((0, 2, 3, 4)), (gm * xh).double().sum((0, 2, 3, 4))]).cpu()
    got = psum.double().sum(0).cpu()
    assert float((got - want).abs().max()) / float(want.abs().max()) < 2e-3
    ws = ops._workspace(1, dev, "splitk")
    assert int(ws[:4096].view(torch.int32).abs().max()) == 0, "arrival counters not cleared"


# name, N, Cin, T, H, W, Cout, k, s, p: shapes for the deep-pipeline kernel (>= 192 columns both directions)
DEEP_CASES = [
    ("s4a_t3_1024_256", 2, 1024, 8, 14, 14, 256, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    ("s4b_3x3_256", 2, 256, 4, 14, 14, 256, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    ("pw_dense_1024_512", 2, 1024, 4, 14, 14, 512, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("pw_strided_640_1024", 2, 640, 4, 14, 14, 1024, (1, 1, 1), (1, 2, 2), (0, 0, 0)),
    ("3x3_strided_256_256", 2, 256, 4, 14, 14, 256, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("ragged_72_264", 3, 72, 3, 13, 11, 264, (1, 3, 3), (1, 1, 1), (0, 1, 1)),   # K = 648 (tail), N = 256 + 8, M = 1287
    ("nk1_64_256", 2, 64, 2, 14, 14, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0)),      # one k-tile: prologue only
    ("nk2_128_256", 2, 128, 2, 14, 14, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("nk3_192_200", 2, 192, 2, 14, 14, 200, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("t5_64_320", 2, 64, 8, 9, 9, 320, (5, 1, 1), (1, 1, 1), (2, 0, 0)),
    ("dg_wide_256_1024", 2, 1024, 4, 14, 14, 256, (3, 1, 1), (1, 1, 1), (1, 0, 0)),  # its dgrad: N = 1024, K = 768
]


@pytest.mark.parametrize("case", DEEP_CASES, ids=[c[0] for c in DEEP_CASES])
def test_deep_pipeline_kernel_fwd_and_dgrad(case, dev, guarded_partials):
    """conv_deep.hip (256 x 256 x 64 tile, 8 waves, sub-buffer ring 7 phases deep): forward with every epilogue
    (BN-stat partials, affine + ReLU, residual into a wider buffer) and the unit-stride data gradient (plain,
    + residual, + masked residual, + the producer's BN-backward sums in both mask forms) against torch and against
    the 128 x 128 tile kernel (VS_CONV_NODEEP) -- pointwise dense / strided, temporal and spatial taps, 1 .. 48
    k-tiles, row / column / reduction tails."""
    from vidsitu_amd import ops

    name, n, cin, t, h, w, cout, k, s, p = case
    g = torch.Generator().manual_seed(83)
    x = rb(torch.randn(n, cin, t, h, w, generator=g))
    wgt = rb(torch.randn(cout, cin, *k, generator=g) / (cin * k[0] * k[1] * k[2]) ** 0.5)
    xa, wa = to_act(x, dev), to_w(wgt, dev)
    ref = F.conv3d(x, wgt, stride=s, padding=p)
    ys = tuple(ref.shape)
    FORCE = _lib.VS_CONV_FORCEDEEP | _lib.VS_CONV_NOHALO | _lib.VS_CONV_NOPW  # (the comparison kernel is the tile kernel)
    assert _plan(ops, tuple(x.shape), ys, cin, cout, k, s, p, 0, FORCE)[4] == 4, "forward did not take the deep kernel"
    kw = dict(halo=False, pw=False)
    y, part = ops.conv_fwd(xa, wa, k, s, p, stats=True, deep="force", **kw)
    assert_close(y, ref, TOL, name + " fwd")
    y0, part0 = ops.conv_fwd(xa, wa, k, s, p, stats=True, deep=False, **kw)
    assert_close(y, y0.float(), 4e-3, name + " fwd vs 128 x 128 tile")
    tot, tot0 = part.double().sum(0).cpu(), part0.double().sum(0).cpu()
    assert part.shape[0] == (ops.act_rows(y) + 255) // 256
    assert torch.allclose(tot, tot0, rtol=2e-3, atol=2e-3 * float(tot0.abs().max()))
    assert torch.allclose(tot[0], ref.double().sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=2e-2)
    assert torch.allclose(tot[1], (ref.double() ** 2).sum(dim=(0, 2, 3, 4)), rtol=2e-3, atol=2e-2)
    # run to run: bit for bit
    y2, part2 = ops.conv_fwd(xa, wa, k, s, p, stats=True, deep="force", **kw)
    assert torch.equal(y2.view(torch.int16), y.view(torch.int16)) and torch.equal(part2, part)
    # folded BN + residual + ReLU into a wider (concat) buffer
    sc = (torch.rand(cout, generator=g) + 0.5).to(dev)
    sh = torch.randn(cout, generator=g).to(dev)
    r = rb(torch.randn(ref.shape, generator=g))
    buf = ops.new_act(ys[0], cout + 16, *ys[2:], dev, zero=True)
    out = ops.channel_slice(buf, 8, cout)
    ops.conv_fwd(xa, wa, k, s, p, out=out, scale=sc, shift=sh, residual=to_act(r, dev), relu=True, deep="force", **kw)
    want = (ref * sc.cpu().view(1, -1, 1, 1, 1) + sh.cpu().view(1, -1, 1, 1, 1) + r).relu()
    assert_close(out, want, TOL, name + " fwd epilogue")
    assert float(buf[:, :8].abs().max()) == 0.0 and float(buf[:, 8 + cout:].abs().max()) == 0.0
    if s != (1, 1, 1) or cin < 192:
        return  # the data gradient of a strided conv is the transposed gather (tile kernel); < 192 columns: not deep
    xg = x.clone().requires_grad_()
    yy = F.conv3d(xg, wgt, stride=s, padding=p)
    dy = rb(torch.randn(yy.shape, generator=g))
    (dx_ref,) = torch.autograd.grad(yy, xg, dy)
    wt = ops.weight_transpose(wa)
    dya = to_act(dy, dev)
    xs = tuple(x.shape)
    assert _plan(ops, xs, ys, cin, cout, k, s, p, 1, FORCE)[4] == 4, "dgrad did not take the deep kernel"
    dx = ops.conv_dgrad(dya, wt, xs, k, s, p, deep="force", **kw)
    assert_close(dx, dx_ref, TOL, name + " dgrad")
    assert_close(dx, ops.conv_dgrad(dya, wt, xs, k, s, p, deep=False, **kw).float(), 2.0 ** -7, name + " dgrad vs tile")
    rr = rb(torch.randn(x.shape, generator=g))
    rra = to_act(rr, dev)
    dxr = ops.conv_dgrad(dya, wt, xs, k, s, p, residual=rra, deep="force", **kw)
    assert_close(dxr, dx_ref + rr, TOL, name + " dgrad + residual")
    rows = ops.act_rows(rra)
    bits = torch.randint(0, 256, (rows, cin // 8), generator=g, dtype=torch.uint8).to(dev)
    keep = _unpack_bits(bits, xs)
    dxm = ops.conv_dgrad(dya, wt, xs, k, s, p, residual=rra, residual_bits=bits, deep="force", **kw)
    assert_close(dxm, dx_ref + torch.where(keep.cpu(), rr, torch.zeros(())), TOL, name + " dgrad + masked residual")
    bn_y = to_act(rb(torch.randn(x.shape, generator=g)), dev)
    mean = (torch.randn(cin, generator=g) * 0.2).to(dev)
    invstd = (torch.rand(cin, generator=g) + 0.5).to(dev)
    gamma, beta = torch.randn(cin, generator=g).to(dev), (torch.randn(cin, generator=g) * 0.3).to(dev)
    dxs, psum = ops.conv_dgrad(dya, wt, xs, k, s, p, bn_stats=(bn_y, mean, invstd, gamma, beta), deep="force", **kw)
    assert psum is not None and psum.shape[0] == (rows + 255) // 256
    assert torch.equal(dxs.view(torch.int16), dx.view(torch.int16))
    v = lambda a: a.view(1, -1, 1, 1, 1)
    xh = (bn_y.float() - v(mean)) * v(invstd)
    gm = torch.where(xh * v(gamma) + v(beta) > 0, dx.float(), torch.zeros((), device=dev))
    want = torch.stack([gm.double().sum((0, 2, 3, 4)), (gm * xh).double().sum((0, 2, 3, 4))]).cpu()
    got = psum.double().sum(0).cpu()
    assert float((got - want).abs().max()) / float(want.abs().max()) < 2e-3
    dxb, psb = ops.conv_dgrad(dya, wt, xs, k, s, p, residual=rra, bn_stats=(bn_y, mean, invstd, None, None, bits),
                              deep="force", **kw)
    assert psb is not None and torch.equal(dxb.view(torch.int16), dxr.view(torch.int16))
    gm = torch.where(keep, dxr.float(), torch.zeros((), device=dev))
    want = torch.stack([gm.double().sum((0, 2, 3, 4)), (gm * xh).double().sum((0, 2, 3, 4))]).cpu()
    assert float((psb.double().sum(0).cpu() - want).abs().max()) / float(want.abs().max()) < 1e-5


def test_batched_wgrad_slab_reduce_is_bitwise_the_per_layer_reduce(dev):
    """ops.WgradBatch: the position-split partials of several layers stay in per-layer slabs and ONE launch
    (vs_wgrad_reduce_batched) sums them -- bit for bit what vs_conv_wgrad's own reduce writes; the device table
    is built once and reused (second round), layers without a split (S = 1) bypass it."""
    from vidsitu_amd import ops

    cases = [WG_CASES[i] for i in range(min(6, len(WG_CASES)))] + [
        ("big_3x3", 2, 64, 4, 28, 28, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
        ("big_pw", 2, 128, 4, 28, 28, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ]
    batch = ops.WgradBatch()
    prepared = []
    for ci, case in enumerate(cases):
        x, w, k, s, p = _mk(case, seed=80 + ci)
        y = F.conv3d(x, w, stride=s, padding=p)
        dya = to_act(rb(torch.randn(y.shape, generator=torch.Generator().manual_seed(90 + ci))), dev)
        xa = to_act(x, dev)
        out = torch.empty((w.shape[0], *k, w.shape[1]), dtype=torch.float32, device=dev).permute(0, 4, 1, 2, 3)
        prepared.append((dya, xa, k, s, p, out))
    for rnd in range(2):
        for dya, xa, k, s, p, out in prepared:
            out.fill_(float("nan"))
            ops.conv_wgrad(dya, xa, k, s, p, out=out, batch=batch)
        n_pending = len(batch.pending)
        batch.flush()
        assert not batch.pending and len(batch.tables) == 1
        for dya, xa, k, s, p, out in prepared:
            want = ops.conv_wgrad(dya, xa, k, s, p)
            assert torch.equal(out, want)
    assert n_pending >= 2, "expected several split layers in the batch"


@pytest.mark.parametrize("S,n", [(2, 4096), (3, 40), (16, 40000), (17, 140000), (22, 262144), (64, 131072), (65, 131072),
                                 (14, 589824), (349, 1024), (1024, 2048)])
def test_slab_reduce_forms_are_bitwise_equal(S, n, dev):
    """vs_wgrad_reduce picks a thread mapping by (S, n) -- one thread per float4 column for S <= 16 and for S <= 64 on
    >= 32 768 columns, 16 slices per column through LDS otherwise -- and promises the slice form's additions in the
    slice form's order.  The batched kernel (vs_wgrad_reduce_batched) always runs the slice form: bit for bit, signs of
    zero and special values included; and against an fp64 sum."""
    from vidsitu_amd import ops
    import ctypes as C

    lib = ops._lib.load()
    g = torch.Generator().manual_seed(1000 + S)
    slabs = (torch.randn(S, n, generator=g) * 3.0)
    slabs[:, : min(n, 64)] = 0.0
    slabs[0, : min(n, 32)] = -0.0          # a column of -0.0 + 0.0 ...: the sign of the sum depends on the form's extra + 0.0
    if n > 200:
        slabs[:, 100:104] = -0.0            # all slabs -0.0
        slabs[S // 2, 150] = float("inf")
        slabs[S - 1, 160] = 1e30
        slabs[0, 160] = -1e30
    slabs = slabs.to(dev)
    a = torch.full((n,), float("nan"), device=dev)
    b = torch.full((n,), float("nan"), device=dev)
    ops._lib.call("vs_wgrad_reduce", ops._ptr(slabs), ops._ptr(a), n, S, ops._stream())
    blocks = int(lib.vs_wgrad_reduce_blocks(n))
    table = torch.tensor([[slabs.data_ptr(), b.data_ptr(), n, S, 0]], dtype=torch.int64, device=dev)
    ops._lib.call("vs_wgrad_reduce_batched", ops._ptr(table), 1, blocks, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"S={S} n={n}: the two forms differ in bits"
    ref = slabs.double().sum(0)
    fin = torch.isfinite(ref)
    err = (a.double() - ref)[fin].abs().max() / slabs.double().abs().sum(0)[fin].max().clamp_min(1.0)
    assert float(err) < 1e-6


# name, N, Cin, T, H, W, Cout, stride   (1x1x1, no padding): shapes the persistent pointwise kernel takes
PW_CASES = [
    ("s2c_64_256", 2, 64, 8, 56, 56, 256, (1, 1, 1)),
    ("s3c_128_512", 2, 128, 8, 28, 28, 512, (1, 1, 1)),
    ("s4c_256_1024", 8, 256, 8, 14, 14, 1024, (1, 1, 1)),
    ("s5c_512_2048", 8, 512, 8, 7, 7, 2048, (1, 1, 1)),
    ("s2sc_80_256", 1, 80, 8, 56, 56, 256, (1, 1, 1)),          # K tail: 80 = 64 + 16
    ("s3sc_320_512_s2", 2, 320, 8, 56, 56, 512, (1, 2, 2)),     # strided rows
    ("s2a_256_64", 2, 256, 8, 56, 56, 64, (1, 1, 1)),
    ("s3a_dgradlike_128_320", 1, 128, 8, 28, 28, 320, (1, 1, 1)),  # columns not a multiple of the slice
    ("ragged_72_200", 3, 72, 5, 13, 11, 200, (1, 1, 1)),         # M % 64 != 0, K % 64 != 0, N % 64 != 0
    ("ragged_s2_136_72", 8, 136, 4, 15, 17, 72, (1, 2, 2)),
]


@pytest.mark.parametrize("case", PW_CASES, ids=[c[0] for c in PW_CASES])
def test_persistent_pointwise_kernel_fwd_and_dgrad(case, dev, guarded_partials):
    """conv_pw.hip (1x1x1 convs with K <= 512: weight slice resident in LDS, activation chunks streamed through an
    LDS-DMA ring across tile boundaries): forward with every epilogue and the unit-stride data gradient with every
    epilogue, against torch and BITWISE against the implicit-GEMM kernel (VS_CONV_NOPW) -- the two kernels run the
    same MFMA sequence per accumulator and share the epilogue."""
    from vidsitu_amd import ops

    name, n, cin, t, h, w, cout, s = case
    k, p = (1, 1, 1), (0, 0, 0)
    g = torch.Generator().manual_seed(83)
    x = rb(torch.randn(n, cin, t, h, w, generator=g))
    wgt = rb(torch.randn(cout, cin, 1, 1, 1, generator=g) / cin ** 0.5)
    xa, wa = to_act(x, dev), to_w(wgt, dev)
    ref = F.conv3d(x, wgt, stride=s)
    ys = tuple(ref.shape)
    bits16 = lambda a: a.view(torch.int16)
    assert _plan(ops, tuple(x.shape), ys, cin, cout, k, s, p, 0, flags=_lib.VS_CONV_FORCEPW)[4] == 3, "forward did not take the pointwise kernel"
    y, part = ops.conv_fwd(xa, wa, k, s, p, stats=True, pw="force")
    assert_close(y, ref, TOL, name + " fwd")
    y0, part0 = ops.conv_fwd(xa, wa, k, s, p, stats=True, pw=False)
    assert torch.equal(bits16(y), bits16(y0))
    tot, tot0 = part.double().sum(0).cpu(), part0.double().sum(0).cpu()
    assert torch.allclose(tot, tot0, rtol=1e-5, atol=1e-5 * float(tot0.abs().max()))
    assert torch.allclose(tot[0], ref.double().sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=2e-2)
    # folded BN + masked residual + ReLU into a wider (concat) buffer
    sc = (torch.rand(cout, generator=g) + 0.5).to(dev)
    sh = torch.randn(cout, generator=g).to(dev)
    r = rb(torch.randn(ref.shape, generator=g))
    ra = to_act(r, dev)
    outs = []
    for pw in ("force", False):
        buf = ops.new_act(ys[0], cout + 16, *ys[2:], dev, zero=True)
        out = ops.channel_slice(buf, 8, cout)
        ops.conv_fwd(xa, wa, k, s, p, out=out, scale=sc, shift=sh, residual=ra, relu=True, pw=pw)
        assert float(buf[:, :8].abs().max()) == 0.0 and float(buf[:, 8 + cout:].abs().max()) == 0.0
        outs.append(out)
    want = (ref * sc.cpu().view(1, -1, 1, 1, 1) + sh.cpu().view(1, -1, 1, 1, 1) + r).relu()
    assert_close(outs[0], want, TOL, name + " fwd epilogue")
    assert torch.equal(bits16(outs[0].contiguous()), bits16(outs[1].contiguous()))
    ya, _ = ops.conv_fwd(xa, wa, k, s, p, scale=sc, shift=sh, relu=True, pw="force")
    yb, _ = ops.conv_fwd(xa, wa, k, s, p, scale=sc, shift=sh, relu=True, pw=False)
    assert torch.equal(bits16(ya), bits16(yb))
    if s != (1, 1, 1):
        return  # the strided data gradient is the transposed-gather kernel's
    # data gradient (a 1x1x1 conv's dgrad is the same GEMM with the transposed weight): rows = input positions
    xg = x.clone().requires_grad_()
    yy = F.conv3d(xg, wgt)
    dy = rb(torch.randn(yy.shape, generator=g))
    (dx_ref,) = torch.autograd.grad(yy, xg, dy)
    wt = ops.weight_transpose(wa)
    dya = to_act(dy, dev)
    if cout <= 512:
        assert _plan(ops, tuple(x.shape), ys, cin, cout, k, s, p, 1, flags=_lib.VS_CONV_FORCEPW)[4] == (3 if cin >= 64 else 0)
    dx = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, pw="force")
    assert_close(dx, dx_ref, TOL, name + " dgrad")
    assert torch.equal(bits16(dx), bits16(ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, pw=False)))
    rr = rb(torch.randn(x.shape, generator=g))
    rra = to_act(rr, dev)
    rows = ops.act_rows(rra)
    bits = torch.randint(0, 256, (rows, cin // 8), generator=g, dtype=torch.uint8).to(dev)
    keep = _unpack_bits(bits, tuple(x.shape))
    dxm = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, residual=rra, residual_bits=bits, pw="force")
    assert_close(dxm, dx_ref + torch.where(keep.cpu(), rr, torch.zeros(())), TOL, name + " dgrad + masked residual")
    assert torch.equal(bits16(dxm), bits16(ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, residual=rra,
                                                          residual_bits=bits, pw=False)))
    # + the BN-backward sums of the unit this dx belongs to
    bn_y = to_act(rb(torch.randn(x.shape, generator=g)), dev)
    mean = (torch.randn(cin, generator=g) * 0.2).to(dev)
    invstd = (torch.rand(cin, generator=g) + 0.5).to(dev)
    gamma, beta = torch.randn(cin, generator=g).to(dev), (torch.randn(cin, generator=g) * 0.3).to(dev)
    dxs, psum = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, bn_stats=(bn_y, mean, invstd, gamma, beta), pw="force")
    assert psum is not None and torch.equal(bits16(dxs), bits16(dx))
    v = lambda a: a.view(1, -1, 1, 1, 1)
    xh = (bn_y.float() - v(mean)) * v(invstd)
    gm = torch.where(xh * v(gamma) + v(beta) > 0, dx.float(), torch.zeros((), device=dev))
    want = torch.stack([gm.double().sum((0, 2, 3, 4)), (gm * xh).double().sum((0, 2, 3, 4))]).cpu()
    assert float((psum.double().sum(0).cpu() - want).abs().max()) / float(want.abs().max()) < 2e-3
    dxr = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, residual=rra, pw="force")
    dxb, psb = ops.conv_dgrad(dya, wt, tuple(x.shape), k, s, p, residual=rra,
                              bn_stats=(bn_y, mean, invstd, None, None, bits), pw="force")
    assert psb is not None and torch.equal(bits16(dxb), bits16(dxr))
    gm = torch.where(keep, dxr.float(), torch.zeros((), device=dev))
    want = torch.stack([gm.double().sum((0, 2, 3, 4)), (gm * xh).double().sum((0, 2, 3, 4))]).cpu()
    assert float((psb.double().sum(0).cpu() - want).abs().max()) / float(want.abs().max()) < 1e-5


# name, N, Cin, T, H, W, Cout, k, s, p : data gradients the small-channel (register-resident weights) kernel takes
DIRECT_BNB_CASES = [
    ("s2b_8_8_3x3", 2, 8, 8, 40, 40, 8, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    ("s2a_32_8_t3", 1, 32, 16, 24, 24, 8, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    ("s2c_8_32_pw", 2, 8, 8, 36, 36, 32, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("s3b_16_16_3x3", 2, 16, 6, 30, 26, 16, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    ("s3b0_16_16_s2", 2, 16, 6, 30, 26, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("s3c_16_64_pw_ragged", 3, 16, 5, 13, 11, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
]


@pytest.mark.parametrize("case", DIRECT_BNB_CASES, ids=[c[0] for c in DIRECT_BNB_CASES])
def test_small_channel_dgrad_emits_bn_backward_sums(case, dev, guarded_partials):
    """conv_direct_kernel<.., BNB>: the data gradient of a small-channel conv also emits the BN-backward sums of the
    unit whose complete dz it is (both mask forms) -- dx bitwise the plain launch, sums = what the separate reduce
    pass computes over the stored dx.  (Opt-in, VS_CONV_DIRECTBNB: slower in the step than the reduce pass.)"""
    from vidsitu_amd import ops

    name, n, cin, t, h, w, cout, k, s, p = case
    g = torch.Generator().manual_seed(97)
    x_shape = (n, cin, t, h, w)
    wgt = rb(torch.randn(cout, cin, *k, generator=g) / (cin * k[0] * k[1] * k[2]) ** 0.5)
    ys = ops.conv_out_shape(x_shape, cout, k, s, p)
    assert _plan(ops, x_shape, ys, cin, cout, k, s, p, 1, flags=0)[4] == 1, "dgrad did not take the small-channel kernel"
    dya = to_act(rb(torch.randn(ys, generator=g)), dev)
    wt = ops.weight_transpose(to_w(wgt, dev))
    bits16 = lambda a: a.view(torch.int16)
    dx = ops.conv_dgrad(dya, wt, x_shape, k, s, p)
    bn_y = to_act(rb(torch.randn(x_shape, generator=g)), dev)
    mean = (torch.randn(cin, generator=g) * 0.2).to(dev)
    invstd = (torch.rand(cin, generator=g) + 0.5).to(dev)
    gamma, beta = torch.randn(cin, generator=g).to(dev), (torch.randn(cin, generator=g) * 0.3).to(dev)
    v = lambda a: a.view(1, -1, 1, 1, 1)
    xh = (bn_y.float() - v(mean)) * v(invstd)
    # no residual: the unit's ReLU mask recomputed from gamma / beta
    dxs, psum = ops.conv_dgrad(dya, wt, x_shape, k, s, p, bn_stats=(bn_y, mean, invstd, gamma, beta), direct_bnb=True)
    assert psum is not None and torch.equal(bits16(dxs), bits16(dx))
    gm = torch.where(xh * v(gamma) + v(beta) > 0, dx.float(), torch.zeros((), device=dev))
    want = torch.stack([gm.double().sum((0, 2, 3, 4)), (gm * xh).double().sum((0, 2, 3, 4))]).cpu()
    assert float((psum.double().sum(0).cpu() - want).abs().max()) / float(want.abs().max()) < 2e-5
    if s != (1, 1, 1):
        return  # (a strided dgrad with a residual does not emit the sums)
    # masked residual + the unit's bit mask
    rr = to_act(rb(torch.randn(x_shape, generator=g)), dev)
    rows = ops.act_rows(rr)
    rbits = torch.randint(0, 256, (rows, cin // 8), generator=g, dtype=torch.uint8).to(dev)
    ubits = torch.randint(0, 256, (rows, cin // 8), generator=g, dtype=torch.uint8).to(dev)
    dxr = ops.conv_dgrad(dya, wt, x_shape, k, s, p, residual=rr, residual_bits=rbits)
    dxb, psb = ops.conv_dgrad(dya, wt, x_shape, k, s, p, residual=rr, residual_bits=rbits,
                              bn_stats=(bn_y, mean, invstd, None, None, ubits), direct_bnb=True)
    assert psb is not None and torch.equal(bits16(dxb), bits16(dxr))
    gm = torch.where(_unpack_bits(ubits, x_shape), dxr.float(), torch.zeros((), device=dev))
    want = torch.stack([gm.double().sum((0, 2, 3, 4)), (gm * xh).double().sum((0, 2, 3, 4))]).cpu()
    assert float((psb.double().sum(0).cpu() - want).abs().max()) / float(want.abs().max()) < 2e-5


@pytest.mark.parametrize("case", [("pw_256_64", 2, 256, 4, 28, 28, 64, (1, 1, 1), (0, 0, 0)),
                                  ("t3_256_64", 1, 256, 8, 14, 14, 64, (3, 1, 1), (1, 0, 0)),
                                  ("pw_64_16_small", 2, 64, 8, 20, 20, 16, (1, 1, 1), (0, 0, 0))],
                         ids=lambda c: c[0])
def test_dgrad_emits_the_sums_of_two_bn_units_fed_by_one_gradient(case, dev, guarded_partials):
    """`vs_dgrad_epilogue.bn_y2 ...`: the conv-a data gradient of the block BEHIND a shortcut block is the complete
    masked output gradient of that block -- of its c unit and of its shortcut unit alike.  One epilogue emits both
    units' BN-backward sums: the same sum(g), each unit's sum(g * xhat); dx and the first unit's sums bitwise the
    single-unit launch."""
    from vidsitu_amd import ops

    name, n, cin, t, h, w, cout, k, p = case
    s = (1, 1, 1)
    g = torch.Generator().manual_seed(131)
    x_shape = (n, cin, t, h, w)
    wgt = rb(torch.randn(cout, cin, *k, generator=g) / (cin * k[0] * k[1] * k[2]) ** 0.5)
    ys = ops.conv_out_shape(x_shape, cout, k, s, p)
    dya = to_act(rb(torch.randn(ys, generator=g)), dev)
    wt = ops.weight_transpose(to_w(wgt, dev))
    rr = to_act(rb(torch.randn(x_shape, generator=g)), dev)
    rows = ops.act_rows(rr)
    rbits = torch.randint(0, 256, (rows, cin // 8), generator=g, dtype=torch.uint8).to(dev)
    ubits = torch.randint(0, 256, (rows, cin // 8), generator=g, dtype=torch.uint8).to(dev)
    y1 = to_act(rb(torch.randn(x_shape, generator=g)), dev)
    y2 = to_act(rb(torch.randn(x_shape, generator=g)), dev)
    m1, m2 = (torch.randn(cin, generator=g) * 0.2).to(dev), (torch.randn(cin, generator=g) * 0.2).to(dev)
    i1, i2 = (torch.rand(cin, generator=g) + 0.5).to(dev), (torch.rand(cin, generator=g) + 0.5).to(dev)
    one = ops.conv_dgrad(dya, wt, x_shape, k, s, p, residual=rr, residual_bits=rbits,
                         bn_stats=(y1, m1, i1, None, None, ubits))
    if one[1] is None:
        pytest.skip("this plan does not emit BN-backward sums")
    dx, p1, p2 = ops.conv_dgrad(dya, wt, x_shape, k, s, p, residual=rr, residual_bits=rbits,
                                bn_stats=(y1, m1, i1, None, None, ubits), bn_stats2=(y2, m2, i2))
    assert p2 is not None and tuple(p2.shape) == tuple(p1.shape)
    assert torch.equal(dx.view(torch.int16), one[0].view(torch.int16)) and torch.equal(p1, one[1])
    assert torch.equal(p2[:, 0], p1[:, 0])  # the same sum(g)
    v = lambda a: a.view(1, -1, 1, 1, 1)
    gm = torch.where(_unpack_bits(ubits, x_shape), dx.float(), torch.zeros((), device=dev))
    xh2 = (y2.float() - v(m2)) * v(i2)
    want = (gm * xh2).double().sum((0, 2, 3, 4)).cpu()
    got = p2[:, 1].double().sum(0).cpu()
    assert float((got - want).abs().max()) / float(want.abs().max()) < 1e-5


# name, N, Cin, T, H, W, Cb, k_b, s_b, p_b, Cc, residual   (conv b -> conv c in one launch, evaluation)
BC_CASES = [
    ("fast_s2", 2, 8, 32, 56, 56, 8, (1, 3, 3), (1, 1, 1), (0, 1, 1), 32, True),
    ("fast_s3", 2, 16, 32, 28, 28, 16, (1, 3, 3), (1, 1, 1), (0, 1, 1), 64, True),
    ("fast_s3_first_stride2", 2, 16, 8, 56, 56, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1), 64, True),
    ("ragged_rows_no_res", 3, 8, 5, 13, 11, 8, (1, 3, 3), (1, 1, 1), (0, 1, 1), 24, False),
    ("temporal_b_16_to_40", 1, 16, 9, 7, 9, 16, (3, 1, 1), (1, 1, 1), (1, 0, 0), 40, True),
    ("wide_in_24", 1, 24, 4, 10, 10, 8, (1, 1, 3), (1, 1, 1), (0, 0, 1), 16, True),
    ("fast_s4_32ch", 2, 32, 8, 14, 14, 32, (1, 3, 3), (1, 1, 1), (0, 1, 1), 128, True),
    ("fast_s4_first_stride2", 1, 32, 4, 28, 28, 32, (1, 3, 3), (1, 2, 2), (0, 1, 1), 128, True),
    ("32ch_ragged_to_72", 3, 32, 3, 9, 7, 32, (1, 3, 3), (1, 1, 1), (0, 1, 1), 72, False),
]


@pytest.mark.parametrize("case", BC_CASES, ids=[c[0] for c in BC_CASES])
def test_fused_bc_eval(case, dev):
    """vs_conv_fwd_bc (conv b + folded BN + ReLU -> conv c + folded BN + residual + ReLU, one launch) against the two
    vs_conv_fwd launches it replaces (same bf16 inner tensor, fp32 residual add: at most one bf16 ulp apart) and
    against torch fp32 on the bf16-rounded operands."""
    from vidsitu_amd import ops

    name, n, cin, t, h, w, cb, k, s, p, cc, with_res = case
    g = torch.Generator().manual_seed(97)
    x = rb(torch.randn(n, cin, t, h, w, generator=g))
    wb = rb(torch.randn(cb, cin, *k, generator=g) / (cin * k[0] * k[1] * k[2]) ** 0.5)
    wc = rb(torch.randn(cc, cb, 1, 1, 1, generator=g) / cb ** 0.5)
    sb, hb = torch.rand(cb, generator=g) + 0.5, torch.randn(cb, generator=g) * 0.2
    s_c, h_c = torch.rand(cc, generator=g) + 0.5, torch.randn(cc, generator=g) * 0.2
    xa, wba, wca = to_act(x, dev), to_w(wb, dev), to_w(wc, dev)
    sbd, hbd, scd, hcd = (v.to(dev) for v in (sb, hb, s_c, h_c))
    assert ops.conv_fwd_bc_fusable(xa, wba, k, s, p, cc)
    yb = F.conv3d(x, wb, stride=s, padding=p)
    res = rb(torch.randn(n, cc, *yb.shape[2:], generator=g)) if with_res else None
    inner = rb(torch.relu(yb * sb.view(1, -1, 1, 1, 1) + hb.view(1, -1, 1, 1, 1)))
    ref = F.conv3d(inner, wc) * s_c.view(1, -1, 1, 1, 1) + h_c.view(1, -1, 1, 1, 1)
    if with_res:
        ref = ref + res
    ref = torch.relu(ref)
    ra = to_act(res, dev) if with_res else None
    got = ops.conv_fwd_bc(xa, wba, k, s, p, sbd, hbd, wca, scd, hcd, residual=ra, relu=True)
    assert_close(got, ref, TOL, name + " fused b->c vs torch")
    b2, _ = ops.conv_fwd(xa, wba, k, s, p, scale=sbd, shift=hbd, relu=True)
    two, _ = ops.conv_fwd(b2, wca, (1, 1, 1), (1, 1, 1), (0, 0, 0), scale=scd, shift=hcd, residual=ra, relu=True)
    assert_close(got, two.float(), 2.0 ** -7, name + " fused b->c vs two launches")
    # into a caller's buffer with a wider row pitch (the trunk writes block outputs into concatenation buffers)
    big = ops.new_act(n, cc + 8, *yb.shape[2:], device=dev)
    big.fill_(7.0)
    view = big[:, :cc]
    ops.conv_fwd_bc(xa, wba, k, s, p, sbd, hbd, wca, scd, hcd, residual=ra, relu=True, out=view)
    assert torch.equal(view, got) and bool((big[:, cc:] == 7.0).all())


def test_fused_bc_refuses_what_it_cannot_take(dev):
    from vidsitu_amd import _lib, ops

    x = to_act(torch.randn(1, 64, 4, 8, 8), dev)
    w64 = to_w(torch.randn(64, 64, 1, 3, 3), dev)  # 64 inner channels, K = 576: the tile kernels' layer
    assert not ops.conv_fwd_bc_fusable(x, w64, (1, 3, 3), (1, 1, 1), (0, 1, 1), 256)
    w8 = to_w(torch.randn(8, 64, 1, 1, 1), dev)  # pointwise conv b
    assert not ops.conv_fwd_bc_fusable(x, w8, (1, 1, 1), (1, 1, 1), (0, 0, 0), 32)
    w16 = to_w(torch.randn(16, 64, 1, 3, 3), dev)  # 16 inner channels but K = 576 does not fit the registers
    assert not ops.conv_fwd_bc_fusable(x, w16, (1, 3, 3), (1, 1, 1), (0, 1, 1), 64)
    wc = to_w(torch.randn(256, 64, 1, 1, 1), dev)
    one = torch.ones(256, device=dev)
    with pytest.raises(_lib.VsError):
        ops.conv_fwd_bc(x, w64, (1, 3, 3), (1, 1, 1), (0, 1, 1), one[:64], one[:64], wc, one, one)


def test_grouped_weight_gradients_vs_torch(dev):
    """vs_conv_wgrad_group: four convolutions of a slow-pathway ResBlock (1x1x1 stride-2 shortcut, [3,1,1], [1,3,3]
    stride 2, 1x1x1) as one launch -- each dW against torch's fp32 weight gradient of the same bf16 operands, and against
    the per-layer launch."""
    from vidsitu_amd import ops

    g = torch.Generator().manual_seed(21)
    specs = [(128, 256, (1, 1, 1), (1, 2, 2), 4, 14), (128, 128, (3, 1, 1), (1, 1, 1), 4, 14),
             (128, 128, (1, 3, 3), (1, 2, 2), 4, 14), (128, 256, (1, 1, 1), (1, 1, 1), 4, 7)]
    items, refs, seps = [], [], []
    for cin, cout, k, s, t, hw in specs:
        p = (k[0] // 2, k[1] // 2, k[2] // 2)
        x = rb(torch.randn(3, cin, t, hw, hw, generator=g))
        w = torch.zeros(cout, cin, *k, requires_grad=True)
        y = F.conv3d(x, w, stride=s, padding=p)
        dy = rb(torch.randn(y.shape, generator=g))
        y.backward(dy)
        refs.append(w.grad)
        xa, dya = to_act(x, dev), to_act(dy, dev)
        dw = torch.empty((cout, *k, cin), dtype=torch.float32, device=dev).permute(0, 4, 1, 2, 3)
        items.append((dya, xa, k, s, p, dw))
        seps.append(ops.conv_wgrad(dya, xa, k, s, p).clone())
    assert ops.conv_wgrad_group_ok(items)
    ops.conv_wgrad_group(items)
    torch.cuda.synchronize()
    for (dya, xa, k, s, p, dw), ref, sep in zip(items, refs, seps):
        assert_close(dw, ref, 2e-3, f"grouped dW {tuple(ref.shape)}")
        assert float((dw - sep).abs().max() / sep.abs().max()) < 1e-5
    again = [it[5].clone() for it in items]
    for it in items:
        it[5].zero_()
    ops.conv_wgrad_group(items)
    torch.cuda.synchronize()
    assert all(torch.equal(a, it[5]) for a, it in zip(again, items))
    # twelve items (three blocks' worth) still go out as one launch; twenty-four are outside the envelope
    ops.conv_wgrad_group(items * 3)
    torch.cuda.synchronize()
    assert all(torch.equal(a, it[5]) or float((a - it[5]).abs().max() / a.abs().max()) < 1e-5 for a, it in zip(again, items))
    assert ops.conv_wgrad_group_ok(items * 3) and not ops.conv_wgrad_group_ok(items * 6)


def test_grouped_weight_gradients_with_xcd_resident_jobs_opt_in(dev):
    """Round 6: VS_WGG_JOBS=1 deals the grouped launch's tiles to the XCDs in full 32-block rounds (profiles/r06_wgrad_jobs.txt;
    half the fabric-side bytes, no time gain -> opt-in).  The switch is read once per process, so the torch comparison above and
    the ResBlock-level grouped test run again in a child process with the switch set: same bounds, same bitwise repeatability."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VS_WGG_JOBS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(root, "tests", "test_gpu_conv.py") + "::test_grouped_weight_gradients_vs_torch",
                        os.path.join(root, "tests", "test_gpu_trunk.py") + "::test_grouped_weight_gradients_of_a_resblock"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-1500:] + r.stderr[-500:]
