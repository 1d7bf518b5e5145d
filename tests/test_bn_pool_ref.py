"""The criteria of tests/bn_pool_ref.py, checked on the CPU: the derived bounds admit correct fp32 code (fused or
separately rounded products) and reject a bf16 store by truncation, which the older max-normalised tolerances
(2e-2 .. 3e-2) let through; the helper restatements agree with torch where torch states the same thing."""
import pytest
import torch

import bn_pool_ref as R

ROWS, C = 257, 72


def _fwd_case():
    g = R.gen(11)
    y = R.rb(torch.randn(ROWS, C, generator=g) * 1.5 + 0.3)
    res = R.rb(torch.randn(ROWS, C, generator=g))
    scale = torch.rand(C, generator=g) + 0.5
    shift = torch.randn(C, generator=g) * 0.3
    return y, res, scale, shift


def _bwd_case():
    g = R.gen(12)
    y = R.rb(torch.randn(ROWS, C, generator=g) * 1.5 + 0.3)
    dz = R.rb(torch.randn(ROWS, C, generator=g))
    mean = torch.randn(C, generator=g) * 0.1 + 0.3
    invstd = 1.0 / (torch.rand(C, generator=g) + 1.0)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    dgamma = torch.randn(C, generator=g) * ROWS ** 0.5
    dbeta = torch.randn(C, generator=g) * ROWS ** 0.5
    return y, dz, mean, invstd, gamma, beta, dgamma, dbeta


def test_bf16_rne_is_the_single_rounding():
    g = R.gen(1)
    x = torch.randn(100000, generator=g) * 3
    assert torch.equal(R.bf16_rne(x.double()), x.to(R.BF16).double())  # fp32 inputs: torch rounds once as well
    # exact ties go to even; one fp64 ulp beside a tie goes to the nearer side (fp64 -> fp32 -> bf16 would not)
    one, ulp = 1.0, 2.0 ** -7
    t = torch.tensor([one + ulp / 2, one + 3 * ulp / 2, one + ulp / 2 + 2.0 ** -52, -(one + ulp / 2), 0.0],
                     dtype=torch.float64)
    want = torch.tensor([one, one + 2 * ulp, one + ulp, -one, 0.0], dtype=torch.float64)
    assert torch.equal(R.bf16_rne(t), want)
    assert float(R.bf16_trunc(torch.tensor([1.0 + 1.9 * ulp])).float()) == 1.0 + ulp


@pytest.mark.parametrize("with_res,relu", [(False, False), (True, True)])
def test_forward_bounds_admit_fp32_code_and_reject_truncation(with_res, relu):
    y, res, scale, shift = _fwd_case()
    r = res if with_res else None
    v64, _, delta = R.bn_apply_ref(y, scale, shift, r)
    sep = y.float() * scale + shift  # product rounded separately
    fused = (y.double() * scale.double() + shift.double()).float()  # one rounding: what an fma stores
    if with_res:
        sep, fused = sep + r.float(), fused + r.float()
    if relu:
        sep, fused = sep.clamp_min(0), fused.clamp_min(0)
    for name, v32 in (("separate", sep), ("fused", fused)):
        s = R.assert_interval(f"cpu bn_apply {name} res={with_res} relu={relu}", v32.to(R.BF16), v64, delta, relu)
        assert s["amb"] <= R.AMB_CAP
    s = R.interval_stats(R.bf16_trunc(fused), v64, delta, relu)
    assert s["bad"] > 0.2 * (0.4 if relu else 1.0) * s["n"], s  # truncation: about half of the non-zero elements
    if relu:
        amb = R.assert_mask("cpu bn_apply mask", fused > 0, v64, delta, stored=fused.to(R.BF16).float())
        assert float(amb.sum()) / amb.numel() <= R.EXCL_CAP


def test_res_aff_inner_rounding_is_admitted_on_both_sides_of_a_tie():
    y, y2, scale, shift = _fwd_case()
    g = R.gen(13)
    sc2, sh2 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    v64, hi, delta = R.bn_apply_ref(y, scale, shift, aff2=(y2, sc2, sh2))
    inner = (y2.double() * sc2.double() + sh2.double()).float().to(R.BF16).float()
    v32 = ((y.double() * scale.double() + shift.double()).float() + inner).clamp_min(0)
    R.assert_interval("cpu bn_apply2", v32.to(R.BF16), v64, delta, True, v64_hi=hi)
    assert R.interval_stats(R.bf16_trunc(v32), v64, delta, True, v64_hi=hi)["bad"] > 0.08 * v32.numel()


@pytest.mark.parametrize("mask", [0, 2])
def test_backward_bounds_admit_fp32_code_and_reject_truncation(mask):
    y, dz, mean, invstd, gamma, beta, dgamma, dbeta = _bwd_case()
    excl = None
    g64 = dz.double()
    if mask == 2:
        m64, dm = R.bn_mask_from_y(y, mean, invstd, gamma, beta)
        m32 = (y.float() - mean) * invstd * gamma + beta
        excl = R.assert_mask("cpu bn_bwd mask from y", m32 > 0, m64, dm)
        g64 = g64 * (m64 > 0)
    v64, delta = R.bn_bwd_apply_ref(g64, y, mean, invstd, gamma, dgamma, dbeta, ROWS)
    g32 = g64.float()
    inv_m = torch.tensor(1.0 / ROWS, dtype=torch.float32)
    xh = (y.float() - mean) * invstd
    folded = (gamma * invstd) * ((g32 - dbeta * inv_m) - xh * (dgamma * inv_m))  # the column-owner kernel's order
    generic = gamma * invstd * (g32 - dbeta * inv_m - xh * dgamma * inv_m)  # the generic kernel's
    for name, v32 in (("folded", folded), ("generic", generic)):
        R.assert_interval(f"cpu bn_bwd_apply {name} mask={mask}", v32.to(R.BF16), v64, delta, exclude=excl)
    s = R.interval_stats(R.bf16_trunc(folded), v64, delta, exclude=excl)
    assert s["bad"] > 0.2 * s["n"], s
    # the sums: the exact sum rounded once passes, a relative error of 1e-5 of sum |terms| does not, and the derived
    # bound is tighter than the 2e-6 of the full-size test
    db64, bb, dg64, bg = R.bn_bwd_sums_ref(g64, y, mean, invstd, ROWS, 8 * 32)
    R.assert_sum("cpu dbeta fp64 rounded once", db64.float(), db64, bb)
    R.assert_sum("cpu dgamma fp64 rounded once", dg64.float(), dg64, bg)
    with pytest.raises(AssertionError):
        R.assert_sum("cpu dbeta off by 1e-5", (db64 + 1e-5 * g64.abs().sum(0)).float(), db64, bb)
    assert bool((bb < 2e-6 * g64.abs().sum(0)).all())


def test_pool_restatements_follow_torch_including_nan():
    g = R.gen(3)
    x = torch.relu(R.rb(torch.randn(2, 8, 2, 7, 5, generator=g)).float())
    y, tap = R.maxpool_hw_ref(x)
    xl, yl = x.permute(0, 2, 3, 4, 1).reshape(4, 7, 5, 8), y.permute(0, 2, 3, 4, 1).reshape(4, 4, 3, 8)
    assert torch.equal(R.first_max_tap(xl, yl), tap.permute(0, 2, 3, 4, 1).reshape(4, 4, 3, 8))
    # backward restatement against autograd (fp64: sums of at most 4 terms are exact enough to compare at 1e-15)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    xr = x.double().requires_grad_(True)
    torch.nn.functional.max_pool3d(xr, (1, 3, 3), (1, 2, 2), (0, 1, 1)).backward(dy)
    dx, ab = R.maxpool_hw_bwd_ref(dy.permute(0, 2, 3, 4, 1).reshape(4, 4, 3, 8),
                                  tap.permute(0, 2, 3, 4, 1).reshape(4, 4, 3, 8), 7, 5)
    assert torch.allclose(dx.view(2, 2, 7, 5, 8).permute(0, 4, 1, 2, 3), xr.grad, rtol=0, atol=1e-14)
    assert bool((ab >= dx.abs() - 1e-14).all())
    # torch's 2x2 pool returns NaN, and the NaN's position, wherever in the window the NaN sits
    for q in range(4):
        z = torch.ones(1, 1, 1, 2, 2)
        z[0, 0, 0, q >> 1, q & 1] = float("nan")
        yq, iq = R.maxpool_hw2_ref(z)
        assert bool(torch.isnan(yq).all()) and int(iq) == q
    z = torch.tensor([3.0, 3.0, 1.0, 3.0]).view(1, 1, 1, 2, 2)
    assert int(R.maxpool_hw2_ref(z)[1]) == 0  # first maximum wins
    yt, it = R.maxpool_t_ref(torch.tensor([1.0, 5.0, 5.0, 2.0]).view(1, 1, 4, 1, 1), 4)
    assert float(yt) == 5.0 and int(it) == 1


def test_bit_helpers_and_patterns():
    g = R.gen(4)
    m = torch.rand(5, 24, generator=g) > 0.5
    assert torch.equal(R.unpack_bits(R.pack_bits(m), 24), m)
    buf = R.nan_filled((3, 32), "cpu")
    assert R.untouched(buf, 8, 16)
    buf[:, 8:24] = 1.0
    assert R.untouched(buf, 8, 16) and not R.untouched(buf, 8, 8)
    buf[1, 24] = float("nan")  # the canonical NaN is not the pattern
    assert not R.untouched(buf, 8, 16)
    a = torch.tensor([1.0, float("nan"), -0.0]).to(R.BF16)
    assert R.same_bits(a, a.clone()) and not R.same_bits(a, torch.tensor([1.0, float("nan"), 0.0]).to(R.BF16))
    assert R.bnb_batches(4097, 2048) == (2, 1) and R.bnb_batches(12289, 2048) == (4, 1) and R.bnb_batches(1, 8) == (1, 256)
    assert R.bna_batches(8193, 2048)[0] == 2 and R.bna_batches(40000, 2048)[0] == 4
