#!/usr/bin/env python3
"""What train-mode dropout costs the RoBERTa encoder of the event-relation models: the p = 0.1 arm against the p = 0
arm of the same run -> profiles/roberta_dropout.json.

roberta-base dimensions, random weights, the shapes of tools/evrel_bench.py (8 videos: `sfpret_evrel` 40 sequences x 60
tokens, `rob_evrel` 32 x 120), fp32, eager launches, one process:
  step      forward + loss + backward + fused Adam through the plugin surface at `mdl.rob_dropout` 0 and 0.1, two
            models built from one seed, `--steps` steps per arm and round between two device events, the arms
            alternating and rotating who goes first; the p = 0 arm is also set beside profiles/evrel_step.json
  attn      vs_attn_pad_fwd / _bwd against their _drop twins alone at both shapes (H = 12, dh = 64)
  site      the residual site LayerNorm(res + m o b) as the model runs it (vs_dropout_add_f32 then
            vs_add_layernorm_fwd; vs_add_layernorm_bwd then vs_dropout_add_f32) at [rows, 768] of both shapes, beside
            the plain vs_add_layernorm pair as the p = 0 yardstick -- and, where the library has it
            (docs/experiments/roberta_fused_ln_site.patch applied), the fused pair vs_add_layernorm_drop_fwd / _bwd
            that lost against the composition (profiles/roberta_dropout_fused_site.json)
  memory    peak allocated bytes of one step per arm (no mask tensor is kept)
Reported: per-round figures, medians, and the p = 0 arm's round-to-round spread (the noise a difference has to exceed).

    python tools/roberta_dropout_bench.py [--rounds 5] [--steps 5] [--launches 200] [--commit ID] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = {"sfpret_evrel": (40, 60), "rob_evrel": (32, 120)}
ARMS = {"p0": 0.0, "p0.1": 0.1}
H, DH = 12, 64


def build(row, p, dev):
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_sf_base import get_head_dim
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval
    from vidsitu_amd.optim import ArenaAdam, ParamArena

    cfg = get_cfg({"task_type": "evrel", "mdl.mdl_name": row, "mdl.rob_mdl_name": "roberta-base",
                   "mdl.rob_dropout": p})
    comm = synth_data.make_comm(cfg)
    batch = synth_data.synth_evrel_batch(comm, 8, n_ann=1, feat_dim=get_head_dim(cfg), seed=7, device=dev)
    sel = get_mdl_loss_eval(cfg)
    torch.manual_seed(0)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev).train()
    loss_fn = sel["loss"](cfg, comm)
    opt = ArenaAdam(ParamArena(mdl, adopt_conv=False), lr=1e-5)

    def step():
        opt.zero_grad()
        loss = loss_fn(mdl(batch), batch)["loss"]
        loss.backward()
        opt.step()
        return loss

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    return step


def timed(fn, n):
    """ms per call of fn over n calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(fns, rounds, n):
    """{name: [ms per call in every round]}: the arms alternate within a round, the first one rotates."""
    for fn in fns.values():
        fn()
        fn()
    out = {k: [] for k in fns}
    names = list(fns)
    for r in range(rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            out[name].append(timed(fns[name], n))
    return out


def summary(per_round, base="p0"):
    med = {k: statistics.median(v) for k, v in per_round.items()}
    res = {"ms_by_round": {k: [round(x, 5) for x in v] for k, v in per_round.items()},
           "median_ms": {k: round(v, 5) for k, v in med.items()},
           base + "_round_to_round_spread_ms": round(max(per_round[base]) - min(per_round[base]), 5)}
    for k in per_round:
        if k != base:
            res[k + "_minus_" + base + "_ms"] = round(med[k] - med[base], 5)
            res[k + "_over_" + base] = round(med[k] / med[base], 4)
    return res


def step_arms(row, dev, rounds, steps, parent):
    fns, peak = {}, {}
    for name, p in ARMS.items():
        fns[name] = build(row, p, dev)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fns[name]()
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated()
        # both models stay alive for the alternating rounds: the second arm's base holds the first arm's model
        peak[name] = {"allocated_before_step": base, "peak_allocated_in_step": top, "step_peak_above_base": top - base}
    res = summary(alternate(fns, rounds, steps))
    r, l = ROWS[row]
    res["sequences_x_tokens"] = [r, l]
    res["peak_memory_bytes"] = peak
    res["peak_growth_bytes"] = peak["p0.1"]["step_peak_above_base"] - peak["p0"]["step_peak_above_base"]
    res["one_attention_mask_bytes"] = r * H * l * l * 4  # what ONE layer's stored fp32 mask would take
    res["one_hidden_mask_bytes"] = r * l * H * DH * 4
    if parent is not None:
        hip = parent["train_step"][row]["hip"]
        res["parent_commit_p0"] = {"median_ms": hip["median_ms"],
                                   "round_to_round_spread_ms": round(max(hip["rounds_ms"]) - min(hip["rounds_ms"]), 4),
                                   "this_p0_minus_parent_ms": round(res["median_ms"]["p0"] - hip["median_ms"], 4)}
    return res


def attn_arms(r, l, dev, rounds, n):
    from vidsitu_amd import ops

    d = H * DH
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(r * l, 3 * d, generator=g).to(dev)
    dout = torch.randn(r * l, d, generator=g).to(dev)
    mask = torch.ones(r, l, dtype=torch.uint8)
    for i in range(r):  # right padding of differing lengths, up to half the sequence (evrel_bench.py's)
        mask[i, l - (i * 7) % (l // 2):] = 0
    mask = mask.to(dev)
    snap = torch.tensor([1234567891011, 5], dtype=torch.int64, device=dev)
    drop = (snap, 1) + ops.dropout_params(0.1)
    fwd = summary(alternate({"p0": lambda: ops.attn_pad(qkv, mask, r, l, H),
                             "p0.1": lambda: ops.attn_pad(qkv, mask, r, l, H, drop=drop)}, rounds, n))
    bwd = summary(alternate({"p0": lambda: ops.attn_pad_bwd(qkv, mask, dout, r, l, H),
                             "p0.1": lambda: ops.attn_pad_bwd(qkv, mask, dout, r, l, H, drop=drop)}, rounds, n))
    return {"shape": {"R": r, "L": l, "H": H, "dh": DH}, "fwd": fwd, "bwd": bwd}


def site_arms(rows, dev, rounds, n):
    from vidsitu_amd import ops

    d = H * DH
    g = torch.Generator().manual_seed(4)
    b, res, dy = (torch.randn(rows, d, generator=g).to(dev) for _ in range(3))
    gamma, beta = torch.ones(d, device=dev), torch.zeros(d, device=dev)
    dg, db = torch.empty(d, device=dev), torch.empty(d, device=dev)
    snap = torch.tensor([1234567891011, 5], dtype=torch.int64, device=dev)
    drop = (snap, 2) + ops.dropout_params(0.1)
    s = ops.dropout_add(b, res, drop)
    y, mean, rstd = ops.add_layernorm_fwd(s, None, gamma, beta, 1e-5)
    fused = hasattr(ops, "add_layernorm_drop_fwd")  # the experiment patch's wrappers

    def comp_fwd():
        return ops.add_layernorm_fwd(ops.dropout_add(b, res, drop), None, gamma, beta, 1e-5)

    def comp_bwd():
        ds = ops.add_layernorm_bwd(dy, s, None, gamma, mean, rstd, dg_out=dg, db_out=db)[0]
        return ds, ops.dropout_add(ds, None, drop)

    fwd_arms = {"composition": comp_fwd,
                "plain_p0": lambda: ops.add_layernorm_fwd(b, res, gamma, beta, 1e-5)}
    bwd_arms = {"composition": comp_bwd,
                "plain_p0": lambda: ops.add_layernorm_bwd(dy, b, res, gamma, mean, rstd, dg_out=dg, db_out=db)}
    if fused:
        fwd_arms["fused"] = lambda: ops.add_layernorm_drop_fwd(b, res, gamma, beta, 1e-5, drop)
        bwd_arms["fused"] = lambda: ops.add_layernorm_drop_bwd(dy, b, res, gamma, mean, rstd, drop, dg_out=dg,
                                                               db_out=db)
    fwd = summary(alternate(fwd_arms, rounds, n), base="composition")
    bwd = summary(alternate(bwd_arms, rounds, n), base="composition")
    pair = {k: round(fwd["median_ms"][k] + bwd["median_ms"][k], 5) for k in fwd_arms}
    out = {"shape": [rows, d], "fwd": fwd, "bwd": bwd, "pair_median_ms": pair}
    if fused:
        out["fused_pair_over_composition_pair"] = round(pair["fused"] / pair["composition"], 4)
    return out


def commit_id():
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                       stderr=subprocess.DEVNULL).strip()
        dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain"], text=True).strip()
        return head + (" + uncommitted changes" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        return "unknown (no git metadata beside the tree)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: ask git)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roberta_dropout.json"))
    args = ap.parse_args()
    if args.rounds < 5 or args.steps < 5 or args.launches < 50:
        sys.exit("at least 5 rounds of at least 5 steps / 50 launches per arm")
    if not torch.cuda.is_available():
        sys.exit("roberta_dropout_bench.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    parent = None
    parent_path = os.path.join(ROOT, "profiles", "evrel_step.json")
    if os.path.exists(parent_path):
        with open(parent_path) as f:
            parent = json.load(f)
    res = {"config": "roberta-base dimensions, random weights, 8 videos, fp32, eager launches; "
                     "mdl.rob_dropout = hidden = attention probability",
           "commit": args.commit or commit_id(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "steps_per_round": args.steps, "launches_per_round": args.launches,
           "unit": "ms per call, device events around a window of calls; arms alternate inside each round",
           "train_step": {}, "attention": [], "residual_site": []}
    for row in ROWS:
        res["train_step"][row] = step_arms(row, dev, args.rounds, args.steps, parent)
        print(row, json.dumps({k: v for k, v in res["train_step"][row].items() if k != "ms_by_round"}), flush=True)
        torch.cuda.empty_cache()
    for r, l in ROWS.values():
        res["attention"].append(attn_arms(r, l, dev, args.rounds, args.launches))
        res["residual_site"].append(site_arms(r * l, dev, args.rounds, args.launches))
        print("attention", json.dumps(res["attention"][-1]["fwd"]["median_ms"]),
              json.dumps(res["attention"][-1]["bwd"]["median_ms"]), flush=True)
        print("residual site", json.dumps(res["residual_site"][-1]["pair_median_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
