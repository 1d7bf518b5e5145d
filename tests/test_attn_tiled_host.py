"""vs_attn_resident_fits without a GPU: the answer that sends an attention launch to the LDS-resident kernels or to the
key-tiled family (vidsitu_amd/ops.py asks it per direction).  It is monotone in L, it answers 1 at every attention
shape the project ran before the tiled family existed -- those launches keep their kernels -- and 0 where the resident
launchers are pinned to refuse."""
import pytest

from vidsitu_amd import _lib

DHS = (16, 32, 48, 64, 80, 128)
L_MAX = 4200


def _fits(causal, l, dh, backward):
    return _lib.load().vs_attn_resident_fits(int(causal), l, dh, int(backward))


@pytest.mark.parametrize("backward", [0, 1])
@pytest.mark.parametrize("causal", [0, 1])
def test_monotone_in_l(causal, backward):
    """1 up to a limit, 0 from there on; the backward's limit is never above the forward's."""
    for dh in DHS:
        ans = [_fits(causal, l, dh, backward) for l in range(1, L_MAX)]
        assert set(ans) <= {0, 1}
        limit = sum(ans)
        assert ans == [1] * limit + [0] * (len(ans) - limit), (causal, dh, backward)
        if not causal and dh in (48, 80):
            assert limit == 0  # the matrix-unit kernels hold 16, 32, 64 and 128 only
        else:
            assert 0 < limit < L_MAX - 1
        if backward:
            assert limit <= sum(_fits(causal, l, dh, 0) for l in range(1, L_MAX))
        print(f"resident limit causal={causal} dh={dh} backward={backward}: L <= {limit}")


def test_every_shape_of_today_stays_resident():
    shapes = {(c, l, 64) for c in (0, 1) for l in (60, 120)} | {(c, 64, 16) for c in (0, 1)}
    # tests/test_gpu_roberta_ops.py
    shapes |= {(0, l, dh) for l in (1, 5, 15, 16, 17, 60, 64, 65, 120) for dh in (32, 64)}
    # tests/test_gpu_gpt2_ops.py (ATTN_CASES and the left_small case)
    shapes |= {(1, 1, 16), (1, 16, 16), (1, 17, 32), (1, 60, 64), (1, 65, 64), (1, 130, 16), (1, 20, 128), (1, 33, 80),
               (1, 24, 64), (1, 20, 16)}
    for causal, l, dh in sorted(shapes):
        for backward in (0, 1):
            assert _fits(causal, l, dh, backward) == 1, (causal, l, dh, backward)


def test_refused_shapes_answer_zero():
    assert _fits(0, 200, 128, 0) == 0
    for causal in (0, 1):
        for backward in (0, 1):
            assert _fits(causal, 4096, 64, backward) == 0
    for bad in ((0, 0, 64, 0), (1, -3, 64, 1), (1, 8, 0, 0)):
        assert _fits(*bad) == 0


def test_limits_at_head_width_64():
    """The figures the documents quote (include/vidsitu_hip.h)."""
    limit = {(c, b): sum(_fits(c, l, 64, b) for l in range(1, L_MAX)) for c in (0, 1) for b in (0, 1)}
    assert limit == {(0, 0): 192, (0, 1): 144, (1, 0): 303, (1, 1): 252}, limit
