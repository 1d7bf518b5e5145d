"""Every convolution of the bench step at the bench step's own size, against fp64 on equal operands.

The 51 distinct convolution geometries of SlowFast-R50 at 8 clips x 32 x 224^2 (tests/bench_shapes.py derives them from
the oracle's module tree), each in three directions, through the entry points and with the flags the trunk uses: the
library's own plan (no tile / ring / halo / pw / deep override), the two stems through the stem entry points.  Operands are
drawn in fp32 and rounded to bf16 once; the kernel and the fp64 tap-loop reference (bench_shapes.conv_ref64 / dgrad_ref64 /
wgrad_ref64, on the GPU) get the same numbers, so whatever is left is the kernel's own arithmetic.  Two operand kinds:
`noise` (everything N(0,1)) and `bn_like` (x = |N(0,1)| + 1: post-ReLU with a large mean; dy with its per-channel mean
removed; weights N(0, 1/K)) -- the structure that makes the narrow layers' sums cancellation-dominated.

Forward and data gradient (bf16 output, fp32 accumulation), no number taken from the kernels:
  * element bound, zero violations: |got - ref| <= 2^-8 |ref| + 1.01 a, a = K 2^-23 S, with S the same operation on
    |x|, |w| and K the reduction length (the worst-case bound gamma_K S of an fp32 sum of K products at unit roundoff
    2^-24, doubled because the MFMA's internal order and rounding are not documented; a correctly rounded bf16 of a value
    within a of ref is within half an ulp <= 2^-8 of it).  Sharp for the narrow layers (K = 8 .. 576), loose for K in
    the thousands, where the next bound carries;
  * aggregate bound: rel_l2(got, ref) <= 1.25 e0 with e0 = rel_l2(bf16(ref), ref) computed from the reference alone
    (1.66e-3 for Gaussian values).  A correct kernel differs from bf16(ref) only where its fp32 accumulator and ref fall
    on different sides of a rounding boundary; such an element's squared error is about 7x an unflipped one's, so 1.25
    admits about 9 % flipped elements -- some thirty times what fp32 accumulation at K = 6 144 produces -- while a
    dropped tap or K-slice, or one wrong row in 200 704, moves the ratio well past it;
  * forward only, the fp32 side: the BN statistic partials summed in fp64 against sum(ref) and sum(ref^2) per channel:
    sum(y^2) to 1e-3 relative (no cancellation), sum(y) to 1e-3 sqrt(P sum(ref^2)) (its Cauchy-Schwarz scale), and every
    float of the partials written;
  * every output starts as NaN and holds none afterwards; for the first row of every plan kind the output is a channel
    slice of a wider NaN buffer whose neighbours stay NaN.
Weight gradient (fp32 output): rel_l2 <= 5e-6 against fp64 (the project's bound at 802 816 positions on cancelling
operands), a second call bitwise the first, no NaN left; and the grouped launches the trunk forms at this batch (slow
res3 [9, 4] items, slow res4 / res5 three-block groups of 9-10) item by item to the same 5e-6.

Rows without a data gradient, because no entry point exists (their input needs no gradient): NO_DGRAD below.
The last test writes the measured figures and `row -> (forward plan, dgrad plan)` to conv_bench_shapes_fp64.json in the
directory VS_RECORD_DIR names (pytest's temporary directory without it); committed as
profiles/conv_bench_shapes_fp64.json.  The plans are a record, not a pin.
Measured when the file was written: e / e0 1.0000000 .. 1.00000004 on every row and direction, worst element 0.996 of its
bound, sum(y^2) within 1.7e-7, weight gradients 1.4e-7 .. 8.8e-7 per unit and 3.2e-7 .. 1.5e-6 grouped; the whole file
takes 9 s."""
import json
import os
import zlib

import pytest
import torch

import bench_shapes as bs
from gpu_utils import BF16

pytestmark = pytest.mark.gpu

ROWS = bs.bench_rows(8)
IDS = [r.name for r in ROWS]
ROW_OF = {name: r for r in ROWS for name in r.names}
NO_DGRAD = ["s1.pathway0_stem.conv", "s1.pathway1_stem.conv"]  # the two stems: ops has no stem data gradient
DG_ROWS = [r for r in ROWS if r.name not in NO_DGRAD]
KINDS = ("noise", "bn_like")
NAN = float("nan")

RECORD = {}      # row name -> direction -> operand kind -> figures (+ "plan")
GROUP_RECORD = {}
WIDE_DONE = {"fwd": set(), "dgrad": set()}  # plan kinds whose output went into a slice of a wider buffer


class _TorchWithNaNEmpty:
    """Stands in for the name `torch` inside vidsitu_amd.ops: every floating-point buffer the wrappers allocate with
    torch.empty (outputs, BN partials, weight gradients) starts as NaN, so an element the kernel did not write shows."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*a, **k):
        t = torch.empty(*a, **k)
        return t.fill_(NAN) if t.is_floating_point() else t


@pytest.fixture
def ops(monkeypatch):
    from vidsitu_amd import ops as real

    monkeypatch.setattr(real, "torch", _TorchWithNaNEmpty())
    return real


@pytest.fixture(autouse=True)
def _free_between_cases(dev):
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _gen(dev, *key):
    return torch.Generator(device=dev).manual_seed(zlib.crc32(repr(key).encode()))


def _act(shape, dev, g, kind, role):
    """bf16 channels-last activation of logical shape [N, C, T, H, W]: drawn in fp32, rounded once."""
    n, c, t, h, w = shape
    v = torch.randn((n, t, h, w, c), generator=g, device=dev)
    if kind == "bn_like":
        v = v.abs_().add_(1.0) if role == "x" else v.sub_(v.mean(dim=(0, 1, 2, 3), keepdim=True))
    return v.to(BF16).permute(0, 4, 1, 2, 3)


def _weight(r, dev, g, kind):
    """bf16 [Cout, Cin, kT, kH, kW] with [Cout][taps][Cin] memory."""
    w = torch.randn((r.cout, *r.k, r.cin), generator=g, device=dev)
    if kind == "bn_like":
        w *= bs.row_k(r) ** -0.5
    return w.to(BF16).permute(0, 4, 1, 2, 3)


def _xs(r):
    return (r.n, r.cin, r.t, r.h, r.w)


def _ys(r):
    return (r.n, r.cout, *bs.row_out(r))


def _plan(ops, r, dgrad, x_ld=None, y_ld=None):
    """vs_conv_plan for the descriptor ops.conv_fwd(stats=True) / ops.conv_dgrad build for this row."""
    import ctypes as C

    if bs.is_stem(r):
        return "stem"
    d = ops.make_desc(_xs(r), x_ld or r.cin, _ys(r), y_ld or r.cout, r.k, r.s, r.p, 0 if dgrad else ops.VS_CONV_STATS)
    out = (C.c_int * 5)()
    assert ops._lib.load().vs_conv_plan(C.byref(d), dgrad, out) == 0
    return list(out)


def _plan_kind(plan):
    return plan if plan == "stem" else plan[4]


def _rec(r, direction, kind, figures):
    RECORD.setdefault(r.name, {}).setdefault(direction, {})[kind] = figures


def _bf16_figures(got, ref, mag, K, plan):
    """The element and aggregate figures of a bf16 result against fp64, and where the worst element sits."""
    got = got.to(torch.float64)
    nan = int(torch.isnan(got).sum())
    err = (got - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + mag * (1.01 * K * 2.0 ** -23)
    inf = torch.full((), float("inf"), dtype=torch.float64, device=got.device)
    share = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, inf, torch.zeros_like(inf)))
    share = torch.nan_to_num(share, nan=float("inf"))
    e0 = bs.rel_l2_64(bs.rb64(ref), ref)
    e = bs.rel_l2_64(torch.nan_to_num(got, nan=0.0), ref)
    flat = share.reshape(-1)  # logical [N, C, T, H, W] order
    i = int(flat.argmax())
    n, c, t, h, w = ref.shape
    idx = []
    for dim in (w, h, t, c, n):
        idx.append(i % dim)
        i //= dim
    wi, hi, ti, ci, ni = idx
    pos = ((ni * t + ti) * h + hi) * w + wi
    tile_rows = plan[0] if isinstance(plan, list) and plan[0] > 0 else 0
    return {"nan": nan, "violations": int((share > 1.0).sum()), "worst_share": float(flat.max()), "e": e, "e0": e0,
            "e_over_e0": e / e0,
            "worst_at": {"position": pos, "n_t_h_w": [ni, ti, hi, wi], "channel": ci,
                         "row_mod_tile": (pos % tile_rows) if tile_rows else None,
                         "got": float(got[ni, ci, ti, hi, wi]), "ref": float(ref[ni, ci, ti, hi, wi])}}


def _assert_bf16(f, what):
    assert f["nan"] == 0, f"{what}: {f['nan']} output elements were never written (NaN pre-fill)"
    assert f["violations"] == 0, (f"{what}: {f['violations']} elements beyond 2^-8 |ref| + 1.01 K 2^-23 S; the worst is "
                                  f"{f['worst_share']:.3g}x its bound at {f['worst_at']}")
    assert f["e_over_e0"] <= 1.25, (f"{what}: rel_l2 {f['e']:.4e} = {f['e_over_e0']:.3f} x the reference's own bf16 "
                                    f"rounding floor {f['e0']:.4e} (> 1.25); worst element {f['worst_at']}")


def _run_fwd(ops, r, xa, wa, out=None):
    if bs.is_stem(r):
        x4 = ops.pack_input(xa, 4)
        wp = ops.pack_stem_weight(wa.float())
        return ops.stem_conv_fwd(x4, wp, r.cout, r.k[0], out=out, stats=True)
    return ops.conv_fwd(xa, wa, r.k, r.s, r.p, out=out, stats=True)


def _wide(ops, shape, dev):
    """A [N, C, ...] channel slice in the middle of a NaN buffer 16 channels wider."""
    n, c, t, h, w = shape
    buf = ops.new_act(n, c + 16, t, h, w, dev)
    buf.fill_(NAN)
    return buf, ops.channel_slice(buf, 8, c)


def _assert_neighbours_untouched(buf, c, what):
    assert bool(torch.isnan(buf[:, :8]).all()) and bool(torch.isnan(buf[:, 8 + c:]).all()), \
        f"{what}: wrote outside its channel slice"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_forward_with_bn_partials_vs_fp64(row, kind, dev, ops):
    r = row
    g = _gen(dev, r.name, kind, "fwd")
    xa, wa = _act(_xs(r), dev, g, kind, "x"), _weight(r, dev, g, kind)
    K, P = bs.row_k(r), bs.row_positions(r)
    ref = bs.conv_ref64(xa, wa, r.s, r.p)
    mag = bs.mag64(bs.conv_ref64, xa, wa, r.s, r.p)
    plan = _plan(ops, r, 0)
    y, part = _run_fwd(ops, r, xa, wa)
    assert tuple(y.shape) == tuple(ref.shape) == _ys(r)
    f = _bf16_figures(y, ref, mag, K, plan)
    # the fp32 side: BN statistic partials
    part_nan = int(torch.isnan(part).sum())
    tot = torch.nan_to_num(part.double(), nan=0.0).sum(0)
    rsum, rsq = ref.sum(dim=(0, 2, 3, 4)), (ref * ref).sum(dim=(0, 2, 3, 4))
    f["sumsq_rel"] = float(((tot[1] - rsq).abs() / rsq).max())
    f["sum_over_scale"] = float(((tot[0] - rsum).abs() / torch.sqrt(P * rsq)).max())
    f["partial_rows"] = int(part.shape[0])
    f["plan"] = plan
    _rec(r, "fwd", kind, f)
    print(f"fwd {r.name} [{kind}] plan {plan} P {P} K {K}: violations {f['violations']} worst share "
          f"{f['worst_share']:.3f} e/e0 {f['e_over_e0']:.4f} (e0 {f['e0']:.3e}) sum(y^2) rel {f['sumsq_rel']:.2e} "
          f"sum(y) / scale {f['sum_over_scale']:.2e} partial NaN {part_nan}")
    what = f"forward {r.name} [{kind}] plan {plan}"
    _assert_bf16(f, what)
    assert part_nan == 0, f"{what}: {part_nan} floats of the BN partials were never written"
    assert f["sumsq_rel"] <= 1e-3, f"{what}: sum(y^2) partials off by {f['sumsq_rel']:.3e} relative"
    assert f["sum_over_scale"] <= 1e-3, f"{what}: sum(y) partials off by {f['sum_over_scale']:.3e} of sqrt(P sum(ref^2))"
    if _plan_kind(plan) not in WIDE_DONE["fwd"]:
        WIDE_DONE["fwd"].add(_plan_kind(plan))
        buf, out = _wide(ops, _ys(r), dev)
        wplan = _plan(ops, r, 0, y_ld=r.cout + 16)
        _run_fwd(ops, r, xa, wa, out=out)
        fw = _bf16_figures(out, ref, mag, K, wplan)
        f["wide_slice"] = {"plan": wplan, "worst_share": fw["worst_share"], "e_over_e0": fw["e_over_e0"]}
        _assert_bf16(fw, what + f" into a channel slice (plan {wplan})")
        _assert_neighbours_untouched(buf, r.cout, what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", DG_ROWS, ids=[r.name for r in DG_ROWS])
def test_data_gradient_vs_fp64(row, kind, dev, ops):
    r = row
    g = _gen(dev, r.name, kind, "dgrad")
    dya, wa = _act(_ys(r), dev, g, kind, "dy"), _weight(r, dev, g, kind)
    K = r.cout * r.k[0] * r.k[1] * r.k[2]
    ref = bs.dgrad_ref64(dya, wa, _xs(r), r.s, r.p)
    mag = bs.mag64(bs.dgrad_ref64, dya, wa, _xs(r), r.s, r.p)
    plan = _plan(ops, r, 1)
    wt = ops.weight_transpose(wa)
    dx = ops.conv_dgrad(dya, wt, _xs(r), r.k, r.s, r.p)
    assert tuple(dx.shape) == _xs(r)
    f = _bf16_figures(dx, ref, mag, K, plan)
    f["plan"] = plan
    _rec(r, "dgrad", kind, f)
    print(f"dgrad {r.name} [{kind}] plan {plan} rows {r.n * r.t * r.h * r.w} K {K}: violations {f['violations']} "
          f"worst share {f['worst_share']:.3f} e/e0 {f['e_over_e0']:.4f} (e0 {f['e0']:.3e})")
    what = f"data gradient {r.name} [{kind}] plan {plan}"
    _assert_bf16(f, what)
    if _plan_kind(plan) not in WIDE_DONE["dgrad"]:
        WIDE_DONE["dgrad"].add(_plan_kind(plan))
        buf, out = _wide(ops, _xs(r), dev)
        wplan = _plan(ops, r, 1, x_ld=r.cin + 16)
        ops.conv_dgrad(dya, wt, _xs(r), r.k, r.s, r.p, out=out)
        fw = _bf16_figures(out, ref, mag, K, wplan)
        f["wide_slice"] = {"plan": wplan, "worst_share": fw["worst_share"], "e_over_e0": fw["e_over_e0"]}
        _assert_bf16(fw, what + f" into a channel slice (plan {wplan})")
        _assert_neighbours_untouched(buf, r.cin, what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_weight_gradient_vs_fp64(row, kind, dev, ops):
    r = row
    g = _gen(dev, r.name, kind, "wgrad")
    xa, dya = _act(_xs(r), dev, g, kind, "x"), _act(_ys(r), dev, g, kind, "dy")
    ref = bs.wgrad_ref64(dya, xa, r.k, r.s, r.p)

    def run():
        if bs.is_stem(r):
            return ops.stem_conv_wgrad(dya, ops.pack_input(xa, 4), r.k[0])
        return ops.conv_wgrad(dya, xa, r.k, r.s, r.p)

    got, again = run(), run()
    assert tuple(got.shape) == tuple(ref.shape)
    nan = int(torch.isnan(got).sum())
    e = bs.rel_l2_64(torch.nan_to_num(got, nan=0.0), ref)
    same = torch.equal(got, again)
    _rec(r, "wgrad", kind, {"rel_l2": e, "nan": nan, "bitwise_repeat": same})
    print(f"wgrad {r.name} [{kind}] P {bs.row_positions(r)}: rel_l2 vs fp64 {e:.3e} NaN {nan} repeat bitwise {same}")
    assert nan == 0, f"{r.name}: {nan} weight-gradient elements were never written"
    assert e <= 5e-6, f"{r.name} [{kind}]: weight gradient rel_l2 {e:.3e} vs fp64 on equal operands"
    assert same, f"{r.name}: a second call differs from the first"


def _block_items(stage, i):
    names = [f"{stage}.pathway0_res{i}.branch2.{u}" for u in "cba"]  # ResBlock.bwd: c, b, a, then the shortcut
    return names + ([f"{stage}.pathway0_res{i}.branch1"] if i == 0 else [])


# the item lists VideoTrunk._backward_stage forms at this batch (ResBlock.group_span = 3, last block first;
# tests/test_gpu_parity_full.py asserts them as [4, 9] for slow res3 and [9, 10, 10] for slow res4 / res5)
GROUPS = {
    "s3_res3_2_1": sum((_block_items("s3", i) for i in (3, 2, 1)), []),
    "s3_res0": _block_items("s3", 0),
    "s4_res5_4_3": sum((_block_items("s4", i) for i in (5, 4, 3)), []),
    "s4_res2_1_0": sum((_block_items("s4", i) for i in (2, 1, 0)), []),
    "s5_res2_1_0": sum((_block_items("s5", i) for i in (2, 1, 0)), []),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("group", list(GROUPS), ids=list(GROUPS))
def test_grouped_weight_gradients_vs_fp64(group, kind, dev, ops):
    names = GROUPS[group]
    assert [len(v) for v in GROUPS.values()] == [9, 4, 9, 10, 10]
    items, refs = [], []
    for j, name in enumerate(names):
        r = ROW_OF[name]
        g = _gen(dev, group, j, kind, "wgrad_group")
        xa, dya = _act(_xs(r), dev, g, kind, "x"), _act(_ys(r), dev, g, kind, "dy")
        dw = torch.full((r.cout, *r.k, r.cin), NAN, dtype=torch.float32, device=dev).permute(0, 4, 1, 2, 3)
        items.append((dya, xa, r.k, r.s, r.p, dw))
        refs.append(bs.wgrad_ref64(dya, xa, r.k, r.s, r.p))
    assert ops.conv_wgrad_group_ok(items), f"{group}: the library would not run these items as one launch"
    ops.conv_wgrad_group(items)
    torch.cuda.synchronize()
    errs = {}
    for j, (name, it, ref) in enumerate(zip(names, items, refs)):
        nan = int(torch.isnan(it[5]).sum())
        assert nan == 0, f"{group} item {j} ({name}): {nan} elements never written"
        errs[f"{j}:{name}"] = bs.rel_l2_64(it[5], ref)
    GROUP_RECORD.setdefault(group, {})[kind] = errs
    print(f"grouped wgrad {group} [{kind}]: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v <= 5e-6}
    assert not bad, f"{group} [{kind}]: items beyond 5e-6 of fp64: {bad}"


def test_plan_coverage_and_record(dev, tmp_path):
    """Which kernel every row takes, from vs_conv_plan alone, and the figures of this session as one JSON file.  When the
    whole sweep ran in this process: the launches saw the plans recorded here, every plan kind the library picks for this
    model at this batch was exercised, and each once into a channel slice of a wider buffer."""
    from vidsitu_amd import ops

    plans = {r.name: {"fwd": _plan(ops, r, 0), "dgrad": None if r.name in NO_DGRAD else _plan(ops, r, 1)} for r in ROWS}
    kinds = {d: sorted({str(_plan_kind(p[d])) for p in plans.values() if p[d] is not None}) for d in ("fwd", "dgrad")}
    for d in ("fwd", "dgrad"):
        assert set(kinds[d]) <= {"stem", "0", "1", "2", "3", "4", "5"}, kinds
    print("plan kinds at the bench batch (stem / 0 tile / 1 direct / 2 halo / 3 pointwise / 4 deep / 5 in-launch split-K): "
          f"{kinds}")
    for name, p in plans.items():
        print(f"  {name}: fwd {p['fwd']} dgrad {p['dgrad']}")
    ran = {d: {n: v[d] for n, v in RECORD.items() if d in v} for d in ("fwd", "dgrad")}
    for d in ("fwd", "dgrad"):
        for name, by_kind in ran[d].items():
            for f in by_kind.values():
                assert f["plan"] == plans[name][d], (name, d, f["plan"], plans[name][d])
    complete = (all(len(ran["fwd"].get(r.name, {})) == len(KINDS) for r in ROWS)
                and all(len(ran["dgrad"].get(r.name, {})) == len(KINDS) for r in DG_ROWS))
    if complete:
        for d in ("fwd", "dgrad"):
            assert {str(k) for k in WIDE_DONE[d]} == set(kinds[d]), (d, WIDE_DONE[d], kinds[d])
    rows = {}
    for r in ROWS:
        rows[r.name] = {"layers": r.count, "cin": r.cin, "t_h_w": [r.t, r.h, r.w], "cout": r.cout, "k": list(r.k),
                        "s": list(r.s), "p": list(r.p), "positions": bs.row_positions(r), "K": bs.row_k(r),
                        "plan": plans[r.name], **RECORD.get(r.name, {})}
        if r.name in NO_DGRAD:
            rows[r.name]["dgrad"] = "no entry point (the stems' input needs no gradient)"
    rec = {"source": "tests/test_gpu_conv_bench_shapes.py (8 clips x 32 x 224^2, SlowFast-R50; fp64 tap-loop reference on "
                     "equal bf16 operands)",
           "bounds": {"element": "|got - ref| <= 2^-8 |ref| + 1.01 K 2^-23 S (worst_share = worst |got - ref| / bound)",
                      "aggregate": "e_over_e0 = rel_l2(got, ref) / rel_l2(bf16(ref), ref) <= 1.25",
                      "bn_partials": "sumsq_rel <= 1e-3; sum_over_scale = |sum - ref| / sqrt(P sum(ref^2)) <= 1e-3",
                      "wgrad": "rel_l2 <= 5e-6, per unit and per item of the grouped launches"},
           "complete_sweep": complete, "plan_kinds": kinds, "rows": rows, "grouped_wgrad": GROUP_RECORD}
    out_dir = os.environ.get("VS_RECORD_DIR") or str(tmp_path)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "conv_bench_shapes_fp64.json")
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(f"record written to {path}")
