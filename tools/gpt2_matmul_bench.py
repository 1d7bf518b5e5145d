#!/usr/bin/env python3
"""What bf16-operand GEMMs buy the GPT-2 decoder's training step: the `matmul="bf16"` arm against the fp32 arm of the
same run.

GPT-2 medium (24 layers, d = 1024, 16 heads) at the generation bench's 50 x 60 tokens, one process:
  step      forward_train + LM loss + backward + fused Adam, eager launches, two models built from one seed,
            `--steps` steps per arm and round between two device events, the arms alternating and rotating who
            goes first
  gemms     every distinct GEMM shape of that step alone through `ops.gemm_nt`, both arms: forward, dx and dW of the
            four projections and of the tied lm_head: ms per call between two device events around `--launches`
            back-to-back calls (launch gaps and the split-K reduce are inside the figure; this is no kernel trace), and
            2 M N K over that time beside the dense peaks of the two matrix-core paths (fp32 157.3, bf16 about 2500
            TFLOP/s)
Reported: per-round figures, medians, and the fp32 arm's round-to-round spread (the noise a difference has to exceed).

    python tools/gpt2_matmul_bench.py [--rounds 5] [--steps 10] [--launches 50] [--out profiles/gpt2_matmul.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

R, L, PAD = 50, 60, 50256
ARMS = ("fp32", "bf16")
PEAK_TFLOPS = {"fp32": 157.3, "bf16": 2500.0}


def build(matmul, dev):
    from vidsitu_amd.hf_gpt2_fseq import GPT2_DIMS, FlatTrainFn, GPT2LMHeadModelHip, lm_loss
    from vidsitu_amd.optim import ArenaAdam, ParamArena

    torch.manual_seed(0)
    mdl = GPT2LMHeadModelHip(*GPT2_DIMS["gpt2-medium"], matmul=matmul).to(dev).train()
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


def summary(per_round, base="fp32"):
    med = {k: statistics.median(v) for k, v in per_round.items()}
    res = {"ms_by_round": {k: [round(x, 5) for x in v] for k, v in per_round.items()},
           "median_ms": {k: round(v, 5) for k, v in med.items()},
           base + "_round_to_round_spread_ms": round(max(per_round[base]) - min(per_round[base]), 5)}
    for k in per_round:
        if k != base:
            res[k + "_minus_" + base + "_ms"] = round(med[k] - med[base], 5)
            res[k + "_over_" + base] = round(med[k] / med[base], 4)
    return res


def step_gemms(t, d, v):
    """{(M, N, K): [uses]} of one training step: y = x W (forward), dx = dy W^T, dW = x^T dy as `gemm_nt` runs them."""
    shapes = {}
    for name, k_in, n_out, per_step in (("c_attn", d, 3 * d, 24), ("attn.c_proj", d, d, 24), ("c_fc", d, 4 * d, 24),
                                        ("mlp.c_proj", 4 * d, d, 24), ("lm_head", d, v, 1)):
        # the tied head's dW is dlogits^T hf ([V, d]); a Conv1D's is x^T dy ([in, out])
        dw = (n_out, k_in, t) if name == "lm_head" else (k_in, n_out, t)
        for kind, mnk in (("fwd", (t, n_out, k_in)), ("dx", (t, k_in, n_out)), ("dW", dw)):
            shapes.setdefault(mnk, []).append(f"{name} {kind} x{per_step}")
    return shapes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default="profiles/gpt2_matmul.json")
    args = ap.parse_args()
    if args.rounds < 5 or args.steps < 5 or args.launches < 20:
        sys.exit("at least 5 rounds of at least 5 steps / 20 launches per arm")
    if not torch.cuda.is_available():
        sys.exit("gpt2_matmul_bench.py measures on a GPU; none is visible")
    from vidsitu_amd import ops
    from vidsitu_amd.hf_gpt2_fseq import GPT2_DIMS

    dev = torch.device("cuda:0")
    # ---- the training step
    steps = {name: build(name, dev) for name in ARMS}
    losses = {name: float(steps[name]()) for name in ARMS}
    step_res = summary(alternate(steps, args.rounds, args.steps))
    step_res["loss_after_three_steps"] = losses
    del steps
    torch.cuda.empty_cache()

    # ---- every distinct GEMM of the step alone
    _, d, _, _, vocab = GPT2_DIMS["gpt2-medium"]
    g = torch.Generator().manual_seed(2)
    gemms, by_arm_ms = [], {a: 0.0 for a in ARMS}
    for (m, n, k), uses in step_gemms(R * L, d, vocab).items():
        x, w = torch.randn(m, k, generator=g).to(dev), torch.randn(n, k, generator=g).to(dev)
        out = torch.empty(m, n, device=dev)
        fns = {a: (lambda a=a: ops.gemm_nt(x, w, out=out, bf16=(a == "bf16"))) for a in ARMS}
        for f in fns.values():
            f()
        res = summary(alternate(fns, args.rounds, args.launches))
        flop = 2.0 * m * n * k
        res["M_N_K"], res["uses_per_step"] = [m, n, k], uses
        res["tflops"] = {a: round(flop / (res["median_ms"][a] * 1e-3) / 1e12, 2) for a in ARMS}
        res["fraction_of_peak"] = {a: round(res["tflops"][a] / PEAK_TFLOPS[a], 4) for a in ARMS}
        count = sum(int(u.rsplit("x", 1)[1]) for u in uses)
        for a in ARMS:
            by_arm_ms[a] += count * res["median_ms"][a]
        gemms.append(res)
        del x, w, out
        torch.cuda.empty_cache()

    res = {
        "config": f"GPT-2 medium, {R} x {L} tokens, eager launches; arms: matmul = fp32 | bf16 (fp32 everything else)",
        "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "steps_per_round": args.steps,
        "launches_per_round": args.launches, "peak_tflops_dense": PEAK_TFLOPS,
        "train_step": step_res, "gemms": gemms,
        "per_step_gemm_ms_from_the_table": {a: round(v, 3) for a, v in by_arm_ms.items()},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
