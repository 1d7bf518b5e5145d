"""The infrastructure of tests/test_gpu_conv_bench_shapes.py, checked without a GPU: the table of convolution geometries
derived from the oracle (against the module count, the published MAC figure and the product's own trunk) and the tap-loop
fp64 reference arithmetic (against torch's fp64 convolution and its autograd on every (k, s, p) class of the table)."""
from collections import Counter

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import bench_shapes as bs
from gpu_utils import rb


def test_table_has_51_rows_that_cover_every_conv3d_of_the_oracle():
    rows = bs.bench_rows(8)
    assert len(rows) == 51
    model, _ = bs.oracle_trunk_on_meta()
    n_conv = sum(1 for m in model.modules() if isinstance(m, nn.Conv3d))
    assert n_conv == 110 and sum(r.count for r in rows) == n_conv
    assert len({n for r in rows for n in r.names}) == n_conv  # every layer in exactly one row
    first, last = rows[0], max(rows, key=bs.row_k)
    by_pos = max(rows, key=bs.row_positions)
    assert (by_pos.cin, by_pos.t, by_pos.h, by_pos.w, by_pos.cout, by_pos.k, by_pos.s) == \
        (3, 32, 224, 224, 8, (5, 7, 7), (1, 2, 2)) and bs.row_positions(by_pos) == 3211264
    assert (last.cin, last.t, last.h, last.w, last.cout, last.k) == (2048, 8, 7, 7, 512, (3, 1, 1))
    assert bs.row_positions(last) == 3136 and bs.row_k(last) == 6144
    assert bs.is_stem(first) and sum(1 for r in rows if bs.is_stem(r)) == 2
    assert sum(1 for r in rows if "conv_f2s" in r.name) == 4
    assert round(sum(bs.row_macs(r) for r in rows) / 1e9, 2) == 225.46


def test_table_macs_equal_the_oracles_own_count():
    from oracle.slowfast_ref import count_conv_macs_params

    rows = bs.bench_rows(1)
    model, _ = bs.oracle_trunk_on_meta()
    fast = torch.empty(1, 3, 32, 224, 224, device="meta")
    macs, _ = count_conv_macs_params(model, [fast[:, :, :8], fast])
    assert sum(bs.row_macs(r) * r.count for r in rows) == macs == 50307661824


def test_the_products_trunk_has_the_oracles_convolutions():
    """Same names, same (Cin, Cout, k, s, p): the table derived from the oracle is the table of the product."""
    ours = bs.product_conv_geometry()
    theirs = {name: (key[0], key[4], key[5], key[6], key[7]) for name, key in bs.oracle_conv_list(8)}
    assert ours == theirs
    assert Counter(ours.values()) == Counter(theirs.values())


# one small shape per (k, s, p) class of the table, odd H / W included: Cin, T, H, W, Cout, k, s, p
REF_CASES = [
    ("pw_dense", 5, 3, 6, 7, 4, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ("pw_stride2", 6, 2, 7, 9, 5, (1, 1, 1), (1, 2, 2), (0, 0, 0)),
    ("t3", 4, 5, 5, 3, 6, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    ("s3", 3, 2, 7, 6, 5, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    ("s3_stride2", 4, 2, 9, 7, 3, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("s3_stride2_even", 4, 2, 8, 10, 3, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("f2s_t7_stride4", 3, 16, 3, 5, 6, (7, 1, 1), (4, 1, 1), (3, 0, 0)),
    ("stem_slow", 3, 2, 13, 16, 4, (1, 7, 7), (1, 2, 2), (0, 3, 3)),
    ("stem_fast", 3, 6, 12, 11, 2, (5, 7, 7), (1, 2, 2), (2, 3, 3)),
]


def test_ref_cases_cover_every_geometry_class_of_the_table():
    assert {(r.k, r.s, r.p) for r in bs.bench_rows(8)} == {(c[6], c[7], c[8]) for c in REF_CASES}


@pytest.mark.parametrize("case", REF_CASES, ids=[c[0] for c in REF_CASES])
def test_tap_loop_reference_equals_torch_fp64(case):
    _, cin, t, h, w, cout, k, s, p = case
    g = torch.Generator().manual_seed(cin * 100 + cout)
    x = torch.randn(2, cin, t, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(cout, cin, *k, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x, wt, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dx, dw = torch.autograd.grad(y, (x, wt), dy)
    xd, wd = x.detach(), wt.detach()
    got_y = bs.conv_ref64(xd, wd, s, p)
    assert tuple(got_y.shape) == tuple(y.shape)
    assert bs.rel_l2_64(got_y, y.detach()) <= 1e-12
    got_dx = bs.dgrad_ref64(dy, wd, tuple(x.shape), s, p)
    assert tuple(got_dx.shape) == tuple(x.shape)
    assert bs.rel_l2_64(got_dx, dx) <= 1e-12
    got_dw = bs.wgrad_ref64(dy, xd, k, s, p)
    assert tuple(got_dw.shape) == tuple(wt.shape)
    assert bs.rel_l2_64(got_dw, dw) <= 1e-12
    # the magnitude sums bound the plain ones, and equal them on non-negative operands
    mag = bs.mag64(bs.conv_ref64, xd, wd, s, p)
    assert bool((mag >= got_y.abs() - 1e-12).all())
    assert bs.rel_l2_64(bs.mag64(bs.conv_ref64, xd.abs(), wd.abs(), s, p), bs.conv_ref64(xd.abs(), wd.abs(), s, p)) == 0.0
    assert bool((bs.mag64(bs.dgrad_ref64, dy, wd, tuple(x.shape), s, p) >= got_dx.abs() - 1e-12).all())
    # bf16 activations in their channels-last layout go in as they are
    xb = rb(xd.float()).to(torch.bfloat16).permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
    assert bs.rel_l2_64(bs.conv_ref64(xb, wd, s, p), F.conv3d(xb.double(), wd, stride=s, padding=p)) <= 1e-12


def test_rounding_floor_of_gaussian_values():
    """e0 = rel_l2(bf16(ref), ref), the yardstick of the sweep's aggregate bound: 1.66e-3 for Gaussian values."""
    ref = torch.randn(1 << 20, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    e0 = bs.rel_l2_64(bs.rb64(ref), ref)
    assert 1.60e-3 < e0 < 1.72e-3, e0
