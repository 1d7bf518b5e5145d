"""The stem bounds of tests/stem_ref.py on the CPU: satisfiable by a correctly rounded result, and each error a stem
kernel can make at a tile tail, a chunk's last frame or an odd last pair is rejected by the check named for it.  Also:
the trunk's stem predicate and ops.stem_supported agree (the GPU side of that agreement, with the entry points, is
tests/test_gpu_stem_edges.py::test_predicate_and_entry_points_agree).

The mutant shape has tails everywhere: N = 2, T = 3, H = 17, W = 35 -> Ho = 9, Wo = 18 (tiles of 8 x 16: one row and two
columns of tail), T odd, kT = 5 (two frames of temporal padding at each end), Cout = 8, N(0,1) operands."""
import pytest
import torch

import bench_shapes as bs
import stem_ref as sr

N, T, H, W, COUT, KT = 2, 3, 17, 35, 8, 5
HO, WO = sr.out_hw(H, W)


def _bf16(v):
    return v.to(torch.bfloat16)


@pytest.fixture(scope="module")
def ops_():
    g = torch.Generator().manual_seed(5)
    x = _bf16(torch.randn((N, T, H, W, 3), generator=g)).permute(0, 4, 1, 2, 3)
    w = _bf16(torch.randn((COUT, KT, 7, 7, 3), generator=g)).permute(0, 4, 1, 2, 3)
    dy = _bf16(torch.randn((N, T, HO, WO, COUT), generator=g)).permute(0, 4, 1, 2, 3)
    ref, a = sr.conv_ref(x, w)
    dw, dw_bound = sr.wgrad_ref(dy, x, KT)
    return {"x": x, "w": w, "dy": dy, "ref": ref, "a": a, "dw": dw, "dw_bound": dw_bound}


def _conv(x, w, p):
    return bs.conv_ref64(x, w, sr.STRIDE, p)


def _exact_partials(ref):
    return torch.stack([sr.tile_sums(ref), sr.tile_sums(ref * ref)], 1).to(torch.float32)


def test_geometry_and_arms():
    assert (HO, WO) == (9, 18) and sr.tiles(HO, WO) == (2, 2)
    assert sr.out_hw(1, 1) == (1, 1) and sr.out_hw(5, 3) == (3, 2) and sr.out_hw(150, 166) == (75, 83)
    assert sr.fwd_arm(8, 5, 2) == "stem_pair_reg_kernel<5>" and sr.fwd_arm(8, 5, 1) == "stem_conv_kernel<1>"
    assert sr.fwd_arm(8, 1, 9) == "stem_conv_kernel<1>" and sr.fwd_arm(40, 3, 5) == "stem_conv_kernel<3>"
    assert sr.wgrad_arm(8, 3, 2) == "stem_wgrad_pair_kernel<3>" and sr.wgrad_arm(8, 3, 1) == "stem_wgrad_kernel<1,11>"
    assert sr.wgrad_arm(64, 1, 5) == "stem_wgrad_kernel<4,4>" and sr.wgrad_arm(32, 5, 5) == "stem_wgrad_kernel<2,18>"


def test_tile_sums_number_rows_like_the_kernels():
    v = torch.arange(N * 2 * T * HO * WO, dtype=torch.float64).view(N, 2, T, HO, WO)
    got = sr.tile_sums(v)
    th, tw = sr.tiles(HO, WO)
    assert tuple(got.shape) == (N * T * th * tw, 2)
    for n in range(N):
        for t in range(T):
            for i in range(th):
                for j in range(tw):
                    row = ((n * T + t) * th + i) * tw + j
                    want = v[n, :, t, i * 8:i * 8 + 8, j * 16:j * 16 + 16].sum(dim=(1, 2))
                    assert torch.equal(got[row], want), (n, t, i, j)


def test_correctly_rounded_results_pass_every_bound(ops_):
    ref, a = ops_["ref"], ops_["a"]
    f = sr.check_bf16(bs.rb64(ref), ref, a)
    assert f["nan"] == 0 and f["violations"] == 0 and f["aggregate_ok"] and f["e_over_e0"] == 1.0, f
    g = torch.Generator().manual_seed(6)
    scale = (torch.rand(COUT, generator=g) + 0.5) * torch.tensor([1.0, -1.0] * (COUT // 2))
    shift = torch.randn(COUT, generator=g)
    for relu in (False, True):
        target, r, allow = sr.affine_ref(ref, a, scale, shift, relu)
        f = sr.check_bf16(bs.rb64(target), target, allow, r)
        assert f["violations"] == 0 and f["aggregate_ok"], (relu, f)
    p = sr.check_partials(_exact_partials(ref), ref, a)
    assert p["shape_ok"] and p["nan"] == 0 and p["violations"] == 0, p
    d = sr.check_wgrad(ops_["dw"].to(torch.float32), ops_["dw"], ops_["dw_bound"])
    assert d["nan"] == 0 and d["violations"] == 0 and d["rel_l2"] <= 5e-6, d


def test_mutant_one_tap_dropped_in_the_last_output_row(ops_):
    x, w, ref, a = ops_["x"], ops_["w"], ops_["ref"], ops_["a"]
    one = torch.zeros_like(w)
    one[:, :, 2, 3, 3] = w[:, :, 2, 3, 3]  # the centre tap: inside the image at every output position
    tap = _conv(x, one, sr.pad(KT))
    mut = ref.clone()
    mut[:, :, :, HO - 1] -= tap[:, :, :, HO - 1]
    f = sr.check_bf16(bs.rb64(mut), ref, a)
    assert f["violations"] > 0 and f["worst_at"]["n_t_ho_wo_c"][2] == HO - 1, f
    assert sr.check_bf16(bs.rb64(mut), ref, a)["worst_share"] > 10, f


def test_mutant_frame_past_the_clip_read_as_frame_zero(ops_):
    x, w, ref, a = ops_["x"], ops_["w"], ops_["ref"], ops_["a"]
    z = torch.zeros_like(x[:, :, :1])
    wrapped = torch.cat([z, z, x, x[:, :, :1], z], 2)  # input frame t = T holds frame 0 (the `tin ? ti : 0` address)
    mut = _conv(wrapped, w, (0, 3, 3))
    assert mut.shape == ref.shape and torch.equal(mut[:, :, 0], ref[:, :, 0])  # output frame 0 does not reach t = T
    f = sr.check_bf16(bs.rb64(mut), ref, a)
    assert f["violations"] > 0 and f["worst_at"]["n_t_ho_wo_c"][1] >= T - 2, f


def test_mutant_frames_swapped_in_the_odd_last_pair(ops_):
    x, w, ref, a = ops_["x"], ops_["w"], ops_["ref"], ops_["a"]
    assert T % 2 == 1  # the last pair is (T - 1, T): its second column computes a frame past the clip
    longer = _conv(torch.cat([x, torch.zeros_like(x[:, :, :1])], 2), w, sr.pad(KT))  # what column j = 1 holds for to = T
    mut = ref.clone()
    mut[:, :, T - 1] = longer[:, :, T]
    f = sr.check_bf16(bs.rb64(mut), ref, a)
    assert f["violations"] > 0 and f["worst_at"]["n_t_ho_wo_c"][1] == T - 1 and not f["aggregate_ok"], f


def test_mutant_tail_position_added_into_a_partial_row(ops_):
    x, w, ref, a = ops_["x"], ops_["w"], ops_["ref"], ops_["a"]
    taller = torch.cat([x, torch.zeros_like(x[:, :, :, :2])], 3)  # the accumulators of output row ho = Ho
    tail = _conv(taller, w, sr.pad(KT))[:, :, :, HO]
    part = _exact_partials(ref).to(torch.float64)
    th, tw = sr.tiles(HO, WO)
    n, t, i, j, wo = 1, 2, th - 1, 0, 5
    row = ((n * T + t) * th + i) * tw + j
    v = tail[n, :, t, wo]
    part[row, 0] += v
    part[row, 1] += v * v
    p = sr.check_partials(part.to(torch.float32), ref, a)
    assert p["nan"] == 0 and p["violations"] > 0 and p["worst_at"]["row"] == row, p
    assert p["violations"] == 2 * COUT and p["worst_share"] > 10, p  # every float of the row, far outside


def test_mutant_partial_row_never_written(ops_):
    ref, a = ops_["ref"], ops_["a"]
    part = _exact_partials(ref)
    part[7] = float("nan")
    p = sr.check_partials(part, ref, a)
    assert p["nan"] == 2 * COUT and p["violations"] == 2 * COUT and p["worst_at"]["row"] == 7, p
    short = sr.check_partials(_exact_partials(ref)[:-1], ref, a)
    assert not short["shape_ok"] and short["violations"] > 0


def test_mutant_one_position_missing_from_the_weight_gradient(ops_):
    x, dy, dw, bound = ops_["x"], ops_["dy"], ops_["dw"], ops_["dw_bound"]
    less = dy.clone()
    less[1, :, T - 1, HO - 1, WO - 1] = 0  # the last position of the tail tile of the last frame
    mut = bs.wgrad_ref64(less, x, (KT, 7, 7), sr.STRIDE, sr.pad(KT))
    d = sr.check_wgrad(mut.to(torch.float32), dw, bound)
    assert d["violations"] > 0 and d["worst_share"] > 100, d


# ---- the trunk's stem predicate and ops.stem_supported --------------------------------------------------------------
def test_supported_set_is_the_twenty_pairs():
    from vidsitu_amd import ops

    want = {(c, k) for c in range(8, 65, 8) for k in (1, 3)} | {(c, 5) for c in (8, 16, 24, 32)}
    got = {(c, k) for c in range(0, 130) for k in range(0, 9) if ops.stem_supported(c, k)}
    assert got == want


def test_is_stem_equals_stem_supported():
    from vidsitu_amd import ops
    from vidsitu_amd.trunk import Conv3dP

    for cout in range(1, 65):
        for kt in (1, 3, 5, 7):
            conv = Conv3dP(3, cout, (kt, 7, 7), (1, 2, 2), (kt // 2, 3, 3))
            assert conv.is_stem == ops.stem_supported(cout, kt), (cout, kt)
    assert not Conv3dP(3, 4, (5, 7, 7), (1, 2, 2), (2, 3, 3)).is_stem  # WIDTH_PER_GROUP 32: fast stem of 4 channels
    # the geometric conditions stay
    assert not Conv3dP(8, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3)).is_stem
    assert not Conv3dP(3, 64, (1, 7, 7), (1, 1, 1), (0, 3, 3)).is_stem
    assert not Conv3dP(3, 64, (3, 7, 7), (1, 2, 2), (0, 3, 3)).is_stem
    assert not Conv3dP(3, 64, (1, 3, 3), (1, 2, 2), (0, 1, 1)).is_stem
