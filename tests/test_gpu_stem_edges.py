"""The stem kernels (vidsitu_amd/csrc/conv_stem.hip) against fp64 at tile tails, chunk tails, odd last pairs and every
(Cout, kT) arm, on equal operands, with the derived bounds of tests/stem_ref.py (docs/stem_parity.md; shown satisfiable
and sharp on the CPU by tests/test_stem_ref.py).  Through ops.pack_input(x, 4), ops.pack_stem_weight, ops.stem_conv_fwd
and ops.stem_conv_wgrad, at VS_STEM_PAIR's default.

Operands are drawn in fp32 and rounded to bf16 once; kernel and reference read the same numbers.  `noise`: everything
N(0,1).  `bn_like`: x = |N(0,1)| + 1, dy with its per-channel mean removed, weights N(0, 1/K).  Every output, partial
buffer, weight gradient and the cached slab workspace starts as NaN, and nothing the checks read may still be NaN.
The partials come through ops._partials, so the row guard (partials_guard.guarded_partials) holds them: every row of the
query written, the four rows behind them untouched.

  (a) every admitted (Cout, kT) pair at N=2, T=5, H=17, W=35 (Ho = 9, Wo = 18: 2 x 2 tiles with tails, T = ST_TC + 1), and
      Cout 8 at kT 3 / 5 with T = 1 (the pair shapes on the generic kernels); the ids name the arms, asserted from the
      dispatch rules;
  (b) a geometry sweep on (64, 1), (8, 5), (8, 1), (32, 3), both operand kinds (GEOMS below says which edge each hits);
  (c) output into / gradient read from a channel slice of a buffer 16 channels wider;
  (d) the row guard, in (a) and (b);
  and the agreement of ops.stem_supported with what the two entry points accept, for Cout 1..64 x kT {1, 3, 5, 7}.
Forward: the element bound and e <= 1.25 e0, plain and with affine + ReLU (scale of both signs); per-row partial bounds.
Weight gradient: the element bound, rel_l2 <= 5e-6, a second call bitwise equal.
The last test writes the measured figures and the file's wall time to stem_edges_fp64.json in the directory
VS_RECORD_DIR names (pytest's temporary directory without it); committed as profiles/stem_edges_fp64.json -- a record,
not a bound."""
import ctypes as C
import json
import os
import time
import zlib

import pytest
import torch

import stem_ref as sr
from gpu_utils import BF16
from partials_guard import guarded_partials  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")
KINDS = ("noise", "bn_like")
RECORD = {"arms": {}, "sweep": {}, "wide": {}, "agreement": {}}
CLOCK = {}


def _conv(nt):
    return f"stem_conv_kernel<{nt}>"


def _wg(mt, ntw):
    return f"stem_wgrad_kernel<{mt},{ntw}>"


# (Cout, kT, T) -> (forward kernel, weight-gradient kernel) at VS_STEM_PAIR = 1, written out from the dispatch rules of
# vs_stem_conv_fwd / vs_stem_conv_wgrad: Cout 8 with kT >= 3 and T >= 2 takes the pair kernels; everything else
# stem_conv_kernel<ceil(Cout / 16)> and stem_wgrad_kernel<ceil(Cout / 16), ceil(14 kT / 4)>.
A_GEOM = (2, 5, 17, 35)
ARMS = {}
for _cout in range(8, 65, 8):
    for _kt, _ntw in ((1, 4), (3, 11), (5, 18)):
        if _kt == 5 and _cout > 32:
            continue  # LDS: not admitted
        _mt = {8: 1, 16: 1, 24: 2, 32: 2, 40: 3, 48: 3, 56: 4, 64: 4}[_cout]
        ARMS[(_cout, _kt, 5)] = (_conv(_mt), _wg(_mt, _ntw))
ARMS[(8, 3, 5)] = ("stem_pair_reg_kernel<3>", "stem_wgrad_pair_kernel<3>")
ARMS[(8, 5, 5)] = ("stem_pair_reg_kernel<5>", "stem_wgrad_pair_kernel<5>")
ARMS[(8, 3, 1)] = (_conv(1), _wg(1, 11))  # T = 1: the fast-pathway shape on the generic kernels
ARMS[(8, 5, 1)] = (_conv(1), _wg(1, 18))
A_CASES = list(ARMS)
A_IDS = [f"c{c}k{k}T{t}-{ARMS[c, k, t][0]}-{ARMS[c, k, t][1]}" for c, k, t in A_CASES]
ADMITTED_FWD = {_conv(i) for i in (1, 2, 3, 4)} | {"stem_pair_reg_kernel<3>", "stem_pair_reg_kernel<5>"}
ADMITTED_WG = ({_wg(m, n) for m in (1, 2) for n in (4, 11, 18)} | {_wg(m, n) for m in (3, 4) for n in (4, 11)}
               | {"stem_wgrad_pair_kernel<3>", "stem_wgrad_pair_kernel<5>"})

# N, T, H, W: the edge each geometry hits
GEOMS = {
    "1x1x1x1": (1, 1, 1, 1),        # window larger than the image, one output, T = 1
    "1x2x5x3": (1, 2, 5, 3),        # Ho = 3, Wo = 2: every tap row partly padding; T = 2, one full pair
    "3x3x17x35": (3, 3, 17, 35),    # N = 3, odd last pair, tails of 1 row and 2 columns
    "1x9x16x32": (1, 9, 16, 32),    # one full tile, no spatial tail; T = 9 = SP_TC + 1 = 2 ST_TC + 1: one-frame chunk
    "2x5x30x66": (2, 5, 30, 66),    # tails of 7 rows and 1 column
    "1x4x18x34": (1, 4, 18, 34),    # even sizes, one more than a tile
    "5x9x150x166": (5, 9, 150, 166),  # 60 tiles with both tails; 900 / 600 items > the 512-block grid: the loop wraps
}
SWEEP_PAIRS = [(64, 1), (8, 5), (8, 1), (32, 3)]
WIDE_PAIRS = [(64, 1), (8, 5)]


class _TorchWithNaNEmpty:
    """Stands in for the name `torch` inside vidsitu_amd.ops: every floating-point buffer the wrappers allocate with
    torch.empty (outputs, weight gradients, packed inputs) starts as NaN, so an element the kernel did not write shows."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*a, **k):
        t = torch.empty(*a, **k)
        return t.fill_(NAN) if t.is_floating_point() else t


@pytest.fixture
def ops(monkeypatch):
    from vidsitu_amd import ops as real

    assert os.environ.get("VS_STEM_PAIR", "1") == "1", "the arms named here are those of the default VS_STEM_PAIR"
    monkeypatch.setattr(real, "torch", _TorchWithNaNEmpty())
    return real


@pytest.fixture(autouse=True)
def _clock(dev):
    """Wall time of the file: from the first test's start to the last finished test's end."""
    CLOCK.setdefault("t0", time.perf_counter())
    yield
    torch.cuda.synchronize()
    CLOCK["t1"] = time.perf_counter()


def _gen(dev, *key):
    return torch.Generator(device=dev).manual_seed(zlib.crc32(repr(key).encode()))


def _act(shape, dev, g, kind, role):
    """bf16 channels-last activation of logical shape [N, C, T, H, W]: drawn in fp32, rounded once."""
    n, c, t, h, w = shape
    v = torch.randn((n, t, h, w, c), generator=g, device=dev)
    if kind == "bn_like":
        v = v.abs_().add_(1.0) if role == "x" else v.sub_(v.mean(dim=(0, 1, 2, 3), keepdim=True))
    return v.to(BF16).permute(0, 4, 1, 2, 3)


def _weight(cout, kt, dev, g, kind):
    w = torch.randn((cout, kt, 7, 7, 3), generator=g, device=dev)
    if kind == "bn_like":
        w *= (147 * kt) ** -0.5
    return w.to(BF16).permute(0, 4, 1, 2, 3)


def _wide(ops, shape, dev, fill):
    """A [N, C, ...] channel slice in the middle of a buffer 16 channels wider, filled with `fill`."""
    n, c, t, h, w = shape
    buf = ops.new_act(n, c + 16, t, h, w, dev)
    buf.fill_(fill)
    return buf, ops.channel_slice(buf, 8, c)


def _assert_bf16(f, what):
    assert f["nan"] == 0, f"{what}: {f['nan']} output elements were never written (NaN pre-fill)"
    assert f["violations"] == 0, (f"{what}: {f['violations']} elements beyond their bound; the worst is "
                                  f"{f['worst_share']:.3g}x its bound at {f['worst_at']}")
    assert f["aggregate_ok"], (f"{what}: rel_l2 {f['e']:.4e} = {f['e_over_e0']:.3f} x the reference's own bf16 rounding "
                               f"floor {f['e0']:.4e} (> 1.25); worst element {f['worst_at']}")


def _forward(ops, dev, cout, kt, geom, kind, wide=False):
    """Forward with statistics, then with affine + ReLU, against fp64; returns the figures."""
    n, t, h, w = geom
    g = _gen(dev, cout, kt, geom, kind, "fwd")
    xa, wa = _act((n, 3, t, h, w), dev, g, kind, "x"), _weight(cout, kt, dev, g, kind)
    sign = torch.where(torch.rand(cout, generator=g, device=dev) < 0.5, -1.0, 1.0)
    sign[0], sign[-1] = 1.0, -1.0  # both signs in every case
    scale = (torch.rand(cout, generator=g, device=dev) + 0.5) * sign
    shift = torch.randn(cout, generator=g, device=dev)
    ref, a = sr.conv_ref(xa, wa)
    ho, wo = sr.out_hw(h, w)
    assert tuple(ref.shape) == (n, cout, t, ho, wo)
    x4 = ops.pack_input(xa, 4)
    wp = ops.pack_stem_weight(wa.float())
    what = f"stem forward ({cout}, {kt}) {geom} [{kind}] {sr.fwd_arm(cout, kt, t)}" + (" into a channel slice" if wide else "")

    buf, out = _wide(ops, ref.shape, dev, NAN) if wide else (None, None)
    y, part = ops.stem_conv_fwd(x4, wp, cout, kt, out=out, stats=True)
    assert tuple(y.shape) == tuple(ref.shape)
    f = sr.check_bf16(y, ref, a)
    p = sr.check_partials(part, ref, a)
    print(f"{what}: violations {f['violations']} worst share {f['worst_share']:.3f} e/e0 {f['e_over_e0']:.6f} "
          f"(e0 {f['e0']:.3e}); partials rows {p['rows']} NaN {p['nan']} violations {p.get('violations')} worst share "
          f"{p.get('worst_share', NAN):.3f}")
    _assert_bf16(f, what)
    assert p["shape_ok"], f"{what}: partials of shape {tuple(part.shape)}, {p['rows']} rows expected"
    assert p["nan"] == 0, f"{what}: {p['nan']} floats of the BN partials were never written"
    assert p["violations"] == 0, (f"{what}: {p['violations']} partial sums beyond their bound; the worst is "
                                  f"{p['worst_share']:.3g}x at {p['worst_at']}")
    if wide:
        assert bool(torch.isnan(buf[:, :8]).all()) and bool(torch.isnan(buf[:, 8 + cout:]).all()), \
            f"{what}: wrote outside its channel slice"

    target, r, allow = sr.affine_ref(ref, a, scale, shift, relu=True)
    buf2, out2 = _wide(ops, ref.shape, dev, NAN) if wide else (None, None)
    y2, none = ops.stem_conv_fwd(x4, wp, cout, kt, out=out2, scale=scale, shift=shift, relu=True)
    assert none is None
    f2 = sr.check_bf16(y2, target, allow, r)
    print(f"{what} + affine + ReLU: violations {f2['violations']} worst share {f2['worst_share']:.3f} e/e0 "
          f"{f2['e_over_e0']:.6f}")
    _assert_bf16(f2, what + " + affine + ReLU")
    if wide:
        assert bool(torch.isnan(buf2[:, :8]).all()) and bool(torch.isnan(buf2[:, 8 + cout:]).all()), \
            f"{what} + affine + ReLU: wrote outside its channel slice"
    return {"arm": sr.fwd_arm(cout, kt, t), "element_share": f["worst_share"], "e_over_e0": f["e_over_e0"],
            "affine_relu_element_share": f2["worst_share"], "affine_relu_e_over_e0": f2["e_over_e0"],
            "partial_rows": p["rows"], "partial_sum_share": p["worst_sum_share"],
            "partial_sumsq_share": p["worst_sumsq_share"]}


def _nan_slabs(ops, dev, n, t, h, w, cout, kt):
    """The cached slab workspace the next ops.stem_conv_wgrad of this shape gets, filled with NaN."""
    need = int(ops._lib.load().vs_stem_wgrad_workspace_bytes(n, t, h, w, cout, kt))
    assert need > 0 and need % 4 == 0
    ws = ops._workspace(need, dev)
    ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(NAN)
    return ws


def _wgrad(ops, dev, cout, kt, geom, kind, wide=False):
    n, t, h, w = geom
    ho, wo = sr.out_hw(h, w)
    g = _gen(dev, cout, kt, geom, kind, "wgrad")
    xa, dya = _act((n, 3, t, h, w), dev, g, kind, "x"), _act((n, cout, t, ho, wo), dev, g, kind, "dy")
    ref, bound = sr.wgrad_ref(dya, xa, kt)
    x4 = ops.pack_input(xa, 4)
    dy_in = dya
    if wide:  # dy_ld > Cout, the neighbour channels large and finite: read, they would wreck the bound
        _, dy_in = _wide(ops, dya.shape, dev, 3.0e4)
        dy_in.copy_(dya)
    what = f"stem weight gradient ({cout}, {kt}) {geom} [{kind}] {sr.wgrad_arm(cout, kt, t)}" + \
        (" from a channel slice" if wide else "")
    ws = _nan_slabs(ops, dev, n, t, h, w, cout, kt)
    got = ops.stem_conv_wgrad(dy_in, x4, kt)
    assert ops._workspace(1, dev).data_ptr() == ws.data_ptr()  # the launch read the buffer filled above
    _nan_slabs(ops, dev, n, t, h, w, cout, kt)
    again = ops.stem_conv_wgrad(dy_in, x4, kt)
    assert tuple(got.shape) == tuple(ref.shape) == (cout, 3, kt, 7, 7)
    d = sr.check_wgrad(got, ref, bound)
    same = torch.equal(got, again)
    print(f"{what}: NaN {d['nan']} violations {d['violations']} worst share {d['worst_share']:.3f} rel_l2 "
          f"{d['rel_l2']:.3e} repeat bitwise {same}")
    assert d["nan"] == 0, f"{what}: {d['nan']} elements never written, or summed from a slab no block wrote"
    assert d["violations"] == 0, (f"{what}: {d['violations']} elements beyond 1.01 Kp 2^-23 S; the worst is "
                                  f"{d['worst_share']:.3g}x at {d['worst_at']}")
    assert d["rel_l2"] <= 5e-6, f"{what}: rel_l2 {d['rel_l2']:.3e} vs fp64 on equal operands"
    assert same, f"{what}: a second call differs from the first"
    return {"arm": sr.wgrad_arm(cout, kt, t), "element_share": d["worst_share"], "rel_l2": d["rel_l2"]}


# ---- (a) every arm ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A_CASES, ids=A_IDS)
def test_every_arm_forward(case, dev, ops, guarded_partials):  # noqa: F811
    cout, kt, t = case
    assert ops.stem_supported(cout, kt)
    assert (sr.fwd_arm(cout, kt, t), sr.wgrad_arm(cout, kt, t)) == ARMS[case]
    geom = (A_GEOM[0], t, *A_GEOM[2:])
    RECORD["arms"].setdefault(A_IDS[A_CASES.index(case)], {})["fwd"] = _forward(ops, dev, cout, kt, geom, "noise")
    assert len(guarded_partials) == 1


@pytest.mark.parametrize("case", A_CASES, ids=A_IDS)
def test_every_arm_weight_gradient(case, dev, ops):
    cout, kt, t = case
    assert (sr.fwd_arm(cout, kt, t), sr.wgrad_arm(cout, kt, t)) == ARMS[case]
    geom = (A_GEOM[0], t, *A_GEOM[2:])
    RECORD["arms"].setdefault(A_IDS[A_CASES.index(case)], {})["wgrad"] = _wgrad(ops, dev, cout, kt, geom, "noise")


def test_every_admitted_arm_is_in_the_case_ids():
    from vidsitu_amd import ops

    pairs = {(c, k) for c in range(1, 65) for k in (1, 3, 5, 7) if ops.stem_supported(c, k)}
    assert pairs == {(c, k) for c, k, t in A_CASES if t == 5} and len(pairs) == 20
    assert {v[0] for v in ARMS.values()} == ADMITTED_FWD
    assert {v[1] for v in ARMS.values()} == ADMITTED_WG
    for (c, k, t), (f, g) in ARMS.items():
        i = A_IDS[A_CASES.index((c, k, t))]
        assert f in i and g in i


# ---- (b) geometry sweep -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair", SWEEP_PAIRS, ids=lambda p: f"c{p[0]}k{p[1]}")
@pytest.mark.parametrize("geom", list(GEOMS), ids=list(GEOMS))
def test_geometry_sweep_forward(geom, pair, kind, dev, ops, guarded_partials):  # noqa: F811
    RECORD["sweep"].setdefault(f"c{pair[0]}k{pair[1]}", {}).setdefault(geom, {}).setdefault("fwd", {})[kind] = \
        _forward(ops, dev, *pair, GEOMS[geom], kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair", SWEEP_PAIRS, ids=lambda p: f"c{p[0]}k{p[1]}")
@pytest.mark.parametrize("geom", list(GEOMS), ids=list(GEOMS))
def test_geometry_sweep_weight_gradient(geom, pair, kind, dev, ops):
    RECORD["sweep"].setdefault(f"c{pair[0]}k{pair[1]}", {}).setdefault(geom, {}).setdefault("wgrad", {})[kind] = \
        _wgrad(ops, dev, *pair, GEOMS[geom], kind)


def test_sweep_geometry_hits_the_edges_it_names():
    """The arithmetic behind the comments of GEOMS."""
    grid_cap = 512
    for name, (n, t, h, w) in GEOMS.items():
        ho, wo = sr.out_hw(h, w)
        th, tw = sr.tiles(ho, wo)
        got = {"out": (ho, wo), "tail": (ho % sr.TILE_H, wo % sr.TILE_W), "tiles": th * tw,
               "items": (n * th * tw * -(-t // sr.ST_TC), n * th * tw * -(-t // sr.SP_TC))}
        want = {"1x1x1x1": {"out": (1, 1), "tiles": 1}, "1x2x5x3": {"out": (3, 2)},
                "3x3x17x35": {"tail": (1, 2)}, "1x9x16x32": {"out": (8, 16), "tail": (0, 0), "tiles": 1},
                "2x5x30x66": {"tail": (7, 1)}, "1x4x18x34": {"out": (9, 17)},
                "5x9x150x166": {"out": (75, 83), "tiles": 60, "items": (900, 600)}}[name]
        assert {k: got[k] for k in want} == want, (name, got)
    assert all(i > grid_cap for i in (900, 600))
    assert 9 == sr.SP_TC + 1 == 2 * sr.ST_TC + 1 and A_GEOM[1] == sr.ST_TC + 1


# ---- (c) row ranges of wider buffers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", WIDE_PAIRS, ids=lambda p: f"c{p[0]}k{p[1]}")
def test_forward_into_a_channel_slice(pair, dev, ops):
    RECORD["wide"].setdefault(f"c{pair[0]}k{pair[1]}", {})["fwd"] = \
        _forward(ops, dev, *pair, GEOMS["3x3x17x35"], "noise", wide=True)


@pytest.mark.parametrize("pair", WIDE_PAIRS, ids=lambda p: f"c{p[0]}k{p[1]}")
def test_weight_gradient_from_a_channel_slice(pair, dev, ops):
    RECORD["wide"].setdefault(f"c{pair[0]}k{pair[1]}", {})["wgrad"] = \
        _wgrad(ops, dev, *pair, GEOMS["3x3x17x35"], "noise", wide=True)


# ---- the predicate and the entry points -------------------------------------------------------------------------------
def test_predicate_and_entry_points_agree(dev, ops):
    """ops.stem_supported(cout, kt) is true exactly where both entry points return VS_OK at N=1, T=2, H=W=8 -- and the
    results then meet the bounds; elsewhere both return an error code (raised as VsError) and launch nothing: their
    outputs stay NaN.  The refused calls go to the entry points directly, on buffers wide enough for any Cout <= 64 at
    a pitch of 64, so that nothing but (Cout, kT) is wrong with them."""
    from vidsitu_amd import _lib

    geom = n, t, h, w = (1, 2, 8, 8)
    ho, wo = sr.out_hw(h, w)
    ok, refused = [], []
    g = _gen(dev, "agreement")
    x4 = ops.pack_input(_act((n, 3, t, h, w), dev, g, "noise", "x"), 4)
    wp = torch.zeros((64, 7, 7, 8, 4), dtype=BF16, device=dev)
    dy = torch.zeros((n, t, ho, wo, 64), dtype=BF16, device=dev)
    ws = ops._workspace(1, dev)
    worst = {"fwd": 0.0, "wgrad": 0.0, "partials": 0.0}
    for cout in range(1, 65):
        for kt in (1, 3, 5, 7):
            if ops.stem_supported(cout, kt):
                f = _forward(ops, dev, cout, kt, geom, "noise")
                d = _wgrad(ops, dev, cout, kt, geom, "noise")
                worst["fwd"] = max(worst["fwd"], f["element_share"], f["affine_relu_element_share"])
                worst["partials"] = max(worst["partials"], f["partial_sum_share"], f["partial_sumsq_share"])
                worst["wgrad"] = max(worst["wgrad"], d["element_share"])
                ok.append((cout, kt))
                continue
            y = torch.full((n, t, ho, wo, 64), NAN, dtype=BF16, device=dev)
            part = torch.full((n * t, 2, 64), NAN, dtype=torch.float32, device=dev)
            dw = torch.full((64, 7, 7, 8, 4), NAN, dtype=torch.float32, device=dev)
            with pytest.raises(_lib.VsError):
                _lib.call("vs_stem_conv_fwd", ops._ptr(x4), ops._ptr(wp), ops._ptr(y), n, t, h, w, cout, kt, 64,
                          ops.VS_CONV_STATS, None, None, ops._ptr(part), ops._stream())
            with pytest.raises(_lib.VsError):
                _lib.call("vs_stem_conv_wgrad", ops._ptr(dy), ops._ptr(x4), ops._ptr(dw), n, t, h, w, cout, kt, 64,
                          ops._ptr(ws), C.c_size_t(ws.numel()), ops._stream())
            torch.cuda.synchronize()  # a launch that failed asynchronously would surface here
            assert bool(torch.isnan(y).all()) and bool(torch.isnan(part).all()) and bool(torch.isnan(dw).all()), \
                f"({cout}, {kt}) was refused after something had been launched"
            refused.append((cout, kt))
    assert len(ok) == 20 and len(refused) == 64 * 4 - 20
    RECORD["agreement"] = {"geometry": list(geom), "accepted": ok, "refused": len(refused), "worst_shares": worst}


# ---- record -----------------------------------------------------------------------------------------------------------
def test_record(dev, tmp_path):
    rec = {"source": "tests/test_gpu_stem_edges.py (fp64 tap-loop reference on equal bf16 operands; bounds: "
                     "docs/stem_parity.md)",
           "figures": {"element_share": "worst |got - ref| / bound (asserted <= 1)",
                       "e_over_e0": "rel_l2(got, ref) / rel_l2(bf16(ref), ref) (asserted <= 1.25)",
                       "partial_*_share": "worst |partial - fp64 tile sum| / bound over rows and channels (<= 1)",
                       "rel_l2": "weight gradient against fp64 (asserted <= 5e-6)"},
           "every_arm_geometry": list(A_GEOM), "geometries": {k: list(v) for k, v in GEOMS.items()},
           "wall_seconds": round(CLOCK.get("t1", 0.0) - CLOCK.get("t0", 0.0), 2),
           "complete": (len(RECORD["arms"]) == len(A_CASES) and len(RECORD["sweep"]) == len(SWEEP_PAIRS)
                        and bool(RECORD["agreement"])),
           **RECORD}
    out_dir = os.environ.get("VS_RECORD_DIR") or str(tmp_path)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "stem_edges_fp64.json")
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(f"record written to {path} ({rec['wall_seconds']} s)")
