#!/usr/bin/env python3
"""What train-mode dropout costs the GPT-2 decoder: the p = 0.1 arm against the p = 0 arm of the same run.

GPT-2 medium (24 layers, d = 1024, 16 heads) at the generation bench's 50 x 60 tokens, fp32, one process:
  step      forward_train + LM loss + backward + fused Adam, eager launches, two models built from one seed,
            `--steps` steps per arm and round between two device events, the arms alternating and rotating who
            goes first
  attn      vs_attn_causal_fwd / _bwd against their _drop twins alone at R = 50, L = 60, H = 16, dh = 64
  add       vs_dropout_add_f32 alone at [3000, 1024], beside vs_add_f32 (same bytes, no generator)
  memory    peak allocated bytes of one step per arm (no mask tensor is kept: the arms differ by the residual-site
            temporaries)
Reported: per-round figures, medians, and the p = 0 arm's round-to-round spread (the noise a difference has to exceed).

    python tools/gpt2_dropout_bench.py [--rounds 5] [--steps 10] [--launches 200] [--out profiles/gpt2_dropout.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

R, L, PAD = 50, 60, 50256
ARMS = {"p0": 0.0, "p0.1": 0.1}


def build(p, dev):
    from vidsitu_amd.hf_gpt2_fseq import GPT2_DIMS, FlatTrainFn, GPT2LMHeadModelHip, lm_loss
    from vidsitu_amd.optim import ArenaAdam, ParamArena

    torch.manual_seed(0)
    mdl = GPT2LMHeadModelHip(*GPT2_DIMS["gpt2-medium"], embd_pdrop=p, attn_pdrop=p, resid_pdrop=p).to(dev).train()
    arena = ParamArena(mdl, adopt_conv=False)
    opt = ArenaAdam(arena, lr=1e-5)
    toks = torch.randint(0, PAD, (R, L), generator=torch.Generator().manual_seed(1)).to(dev)
    toks[::7, L - 9:] = PAD  # some right-padded rows, as a batch of captions has
    keep = toks.ne(PAD)

    def step():
        opt.zero_grad()
        tick = torch.zeros(1, device=dev, requires_grad=True)
        loss = lm_loss(FlatTrainFn.apply(mdl, toks, keep, tick), toks, PAD)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default="profiles/gpt2_dropout.json")
    args = ap.parse_args()
    if args.rounds < 5 or args.steps < 5 or args.launches < 50:
        sys.exit("at least 5 rounds of at least 5 steps / 50 launches per arm")
    if not torch.cuda.is_available():
        sys.exit("gpt2_dropout_bench.py measures on a GPU; none is visible")
    from vidsitu_amd import ops

    dev = torch.device("cuda:0")
    # ---- the training step and its peak memory
    steps, peak = {}, {}
    for name, p in ARMS.items():
        steps[name] = build(p, dev)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        steps[name]()
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated()
        # both models stay alive for the alternating rounds: the second arm's base holds the first arm's model
        peak[name] = {"allocated_before_step": base, "peak_allocated_in_step": top, "step_peak_above_base": top - base}
    step_res = summary(alternate(steps, args.rounds, args.steps))
    del steps
    torch.cuda.empty_cache()

    # ---- the attention launches alone
    h, dh = 16, 64
    d = h * dh
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(R * L, 3 * d, generator=g).to(dev)
    dout = torch.randn(R * L, d, generator=g).to(dev)
    km = torch.ones(R, L, dtype=torch.uint8, device=dev)
    km[::7, L - 9:] = 0
    snap = torch.tensor([1234567891011, 5], dtype=torch.int64, device=dev)
    drop = (snap, 1) + ops.dropout_params(0.1)
    attn_fwd = summary(alternate({"p0": lambda: ops.attn_causal(qkv, km, R, L, h),
                                  "p0.1": lambda: ops.attn_causal(qkv, km, R, L, h, drop=drop)},
                                 args.rounds, args.launches))
    attn_bwd = summary(alternate({"p0": lambda: ops.attn_causal_bwd(qkv, km, dout, R, L, h),
                                  "p0.1": lambda: ops.attn_causal_bwd(qkv, km, dout, R, L, h, drop=drop)},
                                 args.rounds, args.launches))

    # ---- the residual-site kernel alone
    x = torch.randn(R * L, d, generator=g).to(dev)
    res = torch.randn(R * L, d, generator=g).to(dev)
    out = torch.empty_like(x)
    drop2 = (snap, 2) + ops.dropout_params(0.1)
    add = summary(alternate({"add_f32": lambda: ops.add_f32(x, res, out=out),
                             "dropout_add_f32": lambda: ops.dropout_add(x, res, drop2, out=out),
                             "dropout_add_f32_no_res": lambda: ops.dropout_add(x, None, drop2, out=out)},
                            args.rounds, args.launches), base="add_f32")
    add_bytes = 3 * x.numel() * 4
    add["bytes_with_res"] = add_bytes
    add["dropout_add_f32_TBps"] = round(add_bytes / (add["median_ms"]["dropout_add_f32"] * 1e-3) / 1e12, 3)

    n_layer = 24
    res = {
        "config": f"GPT-2 medium, {R} x {L} tokens, fp32, eager launches; p = embd = attn = resid",
        "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "steps_per_round": args.steps,
        "launches_per_round": args.launches,
        "train_step": step_res, "peak_memory_bytes": peak,
        "attn_causal_fwd_R50_L60_H16_dh64": attn_fwd, "attn_causal_bwd_R50_L60_H16_dh64": attn_bwd,
        "elementwise_3000x1024": add,
        # per step: 24 forward + 24 backward attention launches; 48 forward residual sites with the residual, 48
        # backward ones and the embedding's without
        "per_step_attention_extra_ms": round(n_layer * (attn_fwd["p0.1_minus_p0_ms"] + attn_bwd["p0.1_minus_p0_ms"]), 4),
        "per_step_elementwise_passes_ms": round(2 * n_layer * add["median_ms"]["dropout_add_f32"]
                                                + (2 * n_layer + 1) * add["median_ms"]["dropout_add_f32_no_res"], 4),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
