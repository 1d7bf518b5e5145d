"""fp64 reference and derived bounds for the stem kernels (vidsitu_amd/csrc/conv_stem.hip): Conv3d(3 -> Cout, [kT,7,7],
stride [1,2,2], pad [kT/2,3,3]) forward with BN statistic partials and a fused affine (+ReLU), and its weight gradient.

The arithmetic is bench_shapes' (conv_ref64 / wgrad_ref64: the definition, tap by tap, in fp64, on whichever device
the operands are on); this module adds the stem's geometry, the numbering of the statistic rows and the bounds.  Every
check returns a dict of figures with the number of violations and where the worst element sits, so a test prints it
and asserts `violations == 0`; nothing here comes from the kernels' output.  docs/stem_parity.md derives the bounds;
tests/test_stem_ref.py shows on the CPU that they are satisfiable and reject the errors a stem kernel can make.

Tensors are logical [N, C, T, Ho, Wo] (fp64 references; kernel outputs in whatever type they have)."""
import torch

import bench_shapes as bs

STRIDE = (1, 2, 2)
TILE_H, TILE_W = 8, 16  # ST_TH x ST_TW: the tile of one statistics row (vs_stem_stats_rows)
ST_TC, SP_TC = 4, 8     # output frames per work item: generic kernels / pair kernels
U23 = 2.0 ** -23        # twice fp32's unit roundoff: the MFMA's internal order and rounding are not documented
SLACK = 1.01


def pad(kt):
    return (kt // 2, 3, 3)


def out_hw(h, w):
    return (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1


def tiles(ho, wo):
    return (ho + TILE_H - 1) // TILE_H, (wo + TILE_W - 1) // TILE_W


def fwd_arm(cout, kt, t, pair_switch=1):
    """The forward kernel vs_stem_conv_fwd launches, from its dispatch rules (VS_STEM_PAIR = 1, the default)."""
    if pair_switch and cout == 8 and kt >= 3 and t >= 2:
        return f"stem_pair_reg_kernel<{kt}>" if pair_switch == 1 else "stem_pair_kernel"
    return f"stem_conv_kernel<{(cout + 15) // 16}>"


def wgrad_arm(cout, kt, t, pair_switch=1):
    """The weight-gradient kernel vs_stem_conv_wgrad launches: the pair kernel, or stem_wgrad_kernel<MT, NTW>."""
    if pair_switch and cout == 8 and kt in (3, 5) and t >= 2:
        return f"stem_wgrad_pair_kernel<{kt}>"
    return f"stem_wgrad_kernel<{(cout + 15) // 16},{(kt * 14 + 3) // 4}>"


def conv_ref(x, w):
    """(ref, a): the fp64 convolution and the accumulation allowance a = K 2^-23 S, K = 3*7*7*kT, S the same sum on
    |x|, |w| (gamma_K S at unit roundoff 2^-24, doubled)."""
    kt = w.shape[2]
    ref = bs.conv_ref64(x, w, STRIDE, pad(kt))
    mag = bs.mag64(bs.conv_ref64, x, w, STRIDE, pad(kt))
    return ref, mag * (3 * 7 * 7 * kt * U23)


def wgrad_ref(dy, x, kt):
    """(ref, bound): the fp64 weight gradient [Cout, 3, kT, 7, 7] and its element bound 1.01 Kp 2^-23 S with
    Kp = N T Ho Wo and S the same sum on |dy|, |x| -- any summation order of Kp exact products, slab reduce included."""
    ref = bs.wgrad_ref64(dy, x, (kt, 7, 7), STRIDE, pad(kt))
    mag = bs.wgrad_ref64(dy.abs(), x.abs(), (kt, 7, 7), STRIDE, pad(kt))
    n, _, t, ho, wo = dy.shape
    return ref, mag * (SLACK * n * t * ho * wo * U23)


def affine_ref(ref, a, scale, shift, relu):
    """(target, allowance) of relu?(ref * scale + shift): the kernel does one fp32 multiply-add on its accumulator
    (within a of ref), so the pre-ReLU value is within a |scale| + 2^-23 (|ref scale| + |shift|) of r = ref scale +
    shift; ReLU is 1-Lipschitz; the bf16 rounding of the result is within 2^-8 |r|."""
    sc = scale.to(torch.float64).view(1, -1, 1, 1, 1)
    sh = shift.to(torch.float64).view(1, -1, 1, 1, 1)
    r = ref * sc + sh
    allow = a * sc.abs() + U23 * ((ref * sc).abs() + sh.abs())
    return (torch.relu(r) if relu else r), r, allow


def _where(flat_index, shape):
    idx = []
    for dim in reversed(shape):
        idx.append(int(flat_index % dim))
        flat_index //= dim
    return idx[::-1]


def _shares(err, bound):
    """err / bound per element; a zero bound admits only a zero error; NaN counts as beyond every bound."""
    inf = torch.full((), float("inf"), dtype=torch.float64, device=err.device)
    share = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, inf, torch.zeros_like(inf)))
    return torch.nan_to_num(share, nan=float("inf"))


def check_bf16(got, target, allow, r=None):
    """A bf16 output against fp64: zero violations of |got - target| <= 2^-8 |r| + 1.01 allow (r = target unless the
    target went through a ReLU), and the aggregate e = rel_l2(got, target) against e0 = rel_l2(bf16(target), target)."""
    got = got.to(torch.float64)
    r = target if r is None else r
    bound = r.abs() * 2.0 ** -8 + allow * SLACK
    share = _shares((got - target).abs(), bound)
    i = int(share.reshape(-1).argmax())
    n, c, t, ho, wo = _where(i, share.shape)
    e0 = bs.rel_l2_64(bs.rb64(target), target)
    e = bs.rel_l2_64(torch.nan_to_num(got, nan=0.0), target)
    return {"nan": int(torch.isnan(got).sum()), "violations": int((share > 1.0).sum()),
            "worst_share": float(share.reshape(-1)[i]), "e": e, "e0": e0, "e_over_e0": e / e0 if e0 > 0 else float(e > 0),
            "aggregate_ok": e <= 1.25 * e0,
            "worst_at": {"n_t_ho_wo_c": [n, t, ho, wo, c], "got": float(got[n, c, t, ho, wo]),
                         "ref": float(target[n, c, t, ho, wo])}}


def tile_sums(v):
    """Per statistics row, the sum of v over the valid positions of the row's 8 x 16 tile: [rows, C] with
    row = ((n T + to) tilesH + th) tilesW + tw, the numbering vs_stem_stats_rows and all forward kernels share."""
    n, c, t, ho, wo = v.shape
    th, tw = tiles(ho, wo)
    full = v.new_zeros((n, c, t, th * TILE_H, tw * TILE_W))
    full[..., :ho, :wo] = v
    s = full.view(n, c, t, th, TILE_H, tw, TILE_W).sum(dim=(4, 6))  # [n, c, t, th, tw]
    return s.permute(0, 2, 3, 4, 1).reshape(n * t * th * tw, c)


def partial_refs(ref, a):
    """(sum, sumsq, bound_sum, bound_sumsq), each [rows, C]: the fp64 tile sums of ref and ref^2 and the bounds on the
    kernels' fp32 sums of their unrounded accumulators v_i (|v_i - ref_i| <= a_i) over the P valid positions of a tile:
      |s - sum ref|   <= 1.01 (sum a_i + P 2^-23 sum |ref_i|)
      |q - sum ref^2| <= 1.01 (sum (2 |ref_i| a_i + a_i^2) + (P + 1) 2^-23 sum (|ref_i| + a_i)^2)"""
    ab = ref.abs()
    p = tile_sums(torch.ones_like(ref[:, :1]))  # [rows, 1]: valid positions of the tile
    bs_ = SLACK * (tile_sums(a) + p * U23 * tile_sums(ab))
    bq = SLACK * (tile_sums(2 * ab * a + a * a) + (p + 1) * U23 * tile_sums((ab + a) ** 2))
    return tile_sums(ref), tile_sums(ref * ref), bs_, bq


def check_partials(part, ref, a):
    """part: [rows, 2, C] fp32 from the kernel.  Every float written (no NaN), each within its bound."""
    s_ref, q_ref, b_s, b_q = partial_refs(ref, a)
    n, c, t, ho, wo = ref.shape
    th, tw = tiles(ho, wo)
    rows = n * t * th * tw
    out = {"rows": rows, "shape_ok": tuple(part.shape) == (rows, 2, c), "nan": int(torch.isnan(part).sum())}
    if not out["shape_ok"]:
        out["violations"] = rows
        return out
    p64 = part.to(torch.float64)
    share = torch.stack([_shares((p64[:, 0] - s_ref).abs(), b_s), _shares((p64[:, 1] - q_ref).abs(), b_q)], 1)
    i = int(share.reshape(-1).argmax())
    row, which, ch = _where(i, share.shape)
    nn, tt, hh, ww = _where(row, (n, t, th, tw))
    out.update({"violations": int((share > 1.0).sum()), "worst_share": float(share.reshape(-1)[i]),
                "worst_sum_share": float(share[:, 0].max()), "worst_sumsq_share": float(share[:, 1].max()),
                "worst_at": {"row": row, "n_t_th_tw": [nn, tt, hh, ww], "c": ch, "which": ("sum", "sumsq")[which],
                             "got": float(p64[row, which, ch]), "ref": float((s_ref, q_ref)[which][row, ch])}})
    return out


def check_wgrad(got, ref, bound):
    """An fp32 weight gradient [Cout, 3, kT, 7, 7] against fp64: zero element violations, rel_l2, NaN count."""
    g64 = got.to(torch.float64)
    share = _shares((g64 - ref).abs(), bound)
    i = int(share.reshape(-1).argmax())
    at = _where(i, share.shape)
    return {"nan": int(torch.isnan(g64).sum()), "violations": int((share > 1.0).sum()),
            "worst_share": float(share.reshape(-1)[i]), "rel_l2": bs.rel_l2_64(torch.nan_to_num(g64, nan=0.0), ref),
            "worst_at": {"co_ci_dt_dh_dw": at, "got": float(g64[tuple(at)]), "ref": float(ref[tuple(at)])}}
