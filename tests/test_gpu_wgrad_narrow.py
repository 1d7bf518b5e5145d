"""Narrow tiles (64 / 32 / 16 output channels) of the register-staged weight-gradient kernel.  The 32- and 16-row
tiles keep the loads of several 64-position steps in flight in registers and refill their position table in halves
without draining the pipeline; the 64-row tiles run the one-step loop.  The LDS images, the step order and the MFMA order are those of the LDS-DMA ring kernel, so `ring=2` is
the bitwise reference; the fp64 bound is the one of test_gpu_conv.py's fast-pathway test (fp32 accumulation and the
fixed-order slab sum leave 1e-7 .. 1e-6; a dropped step, a stale register set or a wrong table half is 1e-2 .. 1)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from gpu_utils import rb, rel_l2, to_act

pytestmark = pytest.mark.gpu

# id -> (BM, BN) as in conv_wgrad.hip's kWgTiles
NARROW_TILES = {2: (64, 128), 3: (64, 64), 4: (32, 128), 5: (32, 64), 6: (16, 128), 7: (16, 64)}
S3 = ((1, 3, 3), (1, 1, 1), (0, 1, 1))

# name: (n, cin, t, h, w, cout, k, s, p)
CASES = {
    # 1 058 positions: ragged last step, Cout under every tile, 72 of 128 columns
    "s3_8_8_23x23": (1, 8, 2, 23, 23, 8, *S3),
    # 144 positions, 16 per frame: both temporal borders inside every step
    "t3_32_8": (3, 32, 3, 4, 4, 8, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    "s3_16_16_stride2": (1, 16, 2, 15, 17, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    "pw_8_32": (1, 8, 2, 23, 23, 32, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    "pw_64_16": (1, 64, 2, 23, 23, 16, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    # a 32-row tile part filled
    "s3_8_24": (1, 8, 2, 23, 23, 24, *S3),
    # fewer steps than the prefetch depth (one block each: <= 512 positions are never split): less than one step, exactly
    # one, and one position more than 64 * (D - 1) for D = 3 and D = 4
    "s3_40pos": (1, 8, 1, 5, 8, 8, *S3),
    "s3_64pos": (1, 8, 1, 8, 8, 8, *S3),
    "s3_129pos": (1, 8, 1, 3, 43, 8, *S3),
    "s3_193pos": (1, 8, 1, 1, 193, 8, *S3),
}
# one block over 2 100 positions = 33 steps, 4.1 table halves, ragged end: 9 column tiles on 8 slots -> no split
LONG = (1, 64, 2, 25, 42, 8, *S3)
LONG_TILE, LONG_SLOTS = 7, 8


@functools.lru_cache(maxsize=None)
def _operands(case, dev):
    """bf16 operands on the GPU and the fp64 weight gradient of the same (rounded) values; computed once per case."""
    n, cin, t, h, w, cout, k, s, p = case
    g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + h)
    x = rb(torch.randn(n, cin, t, h, w, generator=g))
    wt = torch.zeros(cout, cin, *k, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x.double(), wt, stride=s, padding=p)
    dy = rb(torch.randn(y.shape, generator=g))
    (ref,) = torch.autograd.grad(y, wt, dy.double())
    return to_act(x, dev), to_act(dy, dev), ref, k, s, p


@functools.lru_cache(maxsize=None)
def _narrow(case, tile, slots, dev):
    """The kernel under test: register-staged pipeline (ring=1) on a forced narrow tile."""
    from vidsitu_amd import ops

    xa, dya, _, k, s, p = _operands(case, dev)
    out = ops.conv_wgrad(dya, xa, k, s, p, ring=1, tile=tile, slots=slots)
    torch.cuda.synchronize()
    return out


def _id(v):
    return f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v)


GRID = [pytest.param(CASES[c], t, 0, id=f"{c}-{_id(NARROW_TILES[t])}") for c in CASES for t in NARROW_TILES]
GRID.append(pytest.param(LONG, LONG_TILE, LONG_SLOTS, id="long_2100pos-16x64"))


@pytest.mark.parametrize("case,tile,slots", GRID)
def test_narrow_tile_is_bitwise_the_ring(case, tile, slots, dev):
    from vidsitu_amd import ops

    xa, dya, _, k, s, p = _operands(case, dev)
    want = ops.conv_wgrad(dya, xa, k, s, p, ring=2, tile=tile, slots=slots)
    got = _narrow(case, tile, slots, dev)
    assert torch.equal(got, want), f"max diff {float((got - want).abs().max()):.3e}"


@pytest.mark.parametrize("case,tile,slots", GRID)
def test_narrow_tile_vs_fp64_on_equal_bf16_operands(case, tile, slots, dev):
    ref = _operands(case, dev)[2]
    err = rel_l2(_narrow(case, tile, slots, dev).double(), ref)
    print(f"rel_l2 vs fp64 {err:.3e}")
    assert err <= 5e-6, err


@pytest.mark.parametrize("case,tile,slots", GRID)
def test_narrow_tile_is_bitwise_run_to_run(case, tile, slots, dev):
    from vidsitu_amd import ops

    xa, dya, _, k, s, p = _operands(case, dev)
    again = ops.conv_wgrad(dya, xa, k, s, p, ring=1, tile=tile, slots=slots)
    assert torch.equal(again, _narrow(case, tile, slots, dev))


def test_long_case_is_one_block_over_more_than_two_table_refills(dev):
    """The plan the long case relies on: no position split (no slab workspace), so one block walks all 2 100 positions."""
    from vidsitu_amd import _lib, ops

    xa, dya, _, k, s, p = _operands(LONG, dev)
    assert dya.shape[0] * dya.shape[2] * dya.shape[3] * dya.shape[4] == 2100
    for ring in (1, 2):
        # a weight gradient's descriptor shares the ring (16..18) and forced-tile (8..11) fields of the forward flags
        # (the tile id indexes the weight gradient's own table); bits 24..31, block slots / 8, have no name in the header
        flags = _lib.VS_CONV_RING(ring) | _lib.VS_CONV_TILE(LONG_TILE) | ((LONG_SLOTS // 8) << 24)
        d = ops.make_desc(xa.shape, ops.act_ld(xa), dya.shape, ops.act_ld(dya), k, s, p, flags)
        assert _lib.load().vs_conv_wgrad_workspace_bytes(C.byref(d)) == 0
