#!/usr/bin/env python3
"""What bf16-operand GEMMs buy the event-relation training step, and what the K-strided operand forms of the bf16 GEMM
buy on top of them -> profiles/roberta_matmul.json.

RoBERTa-base with random weights and 8 videos, `rob_evrel` (32 sequences x 120 tokens) and `sfpret_evrel` (40 x 60),
the shapes of profiles/evrel_step.json; one process, three arms built from one seed on the same batch:
  fp32          `mdl.rob_matmul=fp32`, the default
  bf16_copies   bf16 operands, the backward through explicit `transpose_f32` copies + `gemm_nt(bf16=True)` (what GPT-2's
                bf16 backward does).  Reachable here only: the step runs with `ops.gemm_bf16` replaced by that
                composition (one transposed copy per tensor and step, as the fp32 backward makes them)
  bf16          `mdl.rob_matmul=bf16`, the shipped mode: `ops.gemm_bf16` reads dy, x and W where they lie
  step    forward + loss + backward + fused Adam, eager launches; `--steps` steps per arm and round between two device
          events, the arms alternating inside each round and rotating who goes first
  gemms   every distinct backward GEMM shape of RoBERTa-base at those token counts alone: the copies' transposes + NT
          call against the single strided call, `--launches` back-to-back calls between two device events (launch gaps
          and the split-K reduce are inside the figure; this is no kernel trace)
Reported: per-round figures, medians, each arm's round-to-round spread (max - min over the rounds), and the keep-or-drop
rule of the strided forms: bf16 beats bf16_copies on both step shapes by more than bf16_copies' own spread.

    python tools/roberta_matmul_bench.py [--rounds 5] [--steps 10] [--launches 30] [--out profiles/roberta_matmul.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("fp32", "bf16_copies", "bf16")
ROWS = {"rob_evrel": (32, 120), "sfpret_evrel": (40, 60)}


def copies_gemm(held):
    """`ops.gemm_bf16` as transposed copies + the NT form.  `held` keeps every tensor transposed in this step (so that
    no address is reused under the cache) with its copy: dqkv and h_in are transposed once for three weight gradients."""
    from vidsitu_amd import ops

    def transposed(t):
        base, rows = t, None
        b = t._base
        if not t.is_contiguous() and b is not None and b.dim() == 2 and b.is_contiguous() and t.stride() == (b.shape[1], 1):
            base, rows = b, (t.storage_offset() - b.storage_offset(), t.shape[1])  # a column range of b
        if id(base) not in held:
            held[id(base)] = (base, ops.transpose_f32(base))
        bt = held[id(base)][1]
        return bt if rows is None else bt[rows[0]:rows[0] + rows[1]]

    def gemm(a, b, bias=None, res=None, act=0, out=None, a_t=False, b_t=False):
        return ops.gemm_nt(transposed(a) if a_t else a, transposed(b) if b_t else b, bias, res, act=act, out=out,
                           bf16=True)

    return gemm


def build(row, arm, dev):
    from vidsitu_amd import ops, synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_sf_base import get_head_dim
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval
    from vidsitu_amd.optim import ArenaAdam, ParamArena

    cfg = get_cfg({"task_type": "evrel", "mdl.mdl_name": row, "mdl.rob_mdl_name": "roberta-base",
                   "mdl.rob_matmul": "fp32" if arm == "fp32" else "bf16"})
    comm = synth_data.make_comm(cfg)
    batch = synth_data.synth_evrel_batch(comm, 8, n_ann=1, feat_dim=get_head_dim(cfg), seed=7, device=dev)
    sel = get_mdl_loss_eval(cfg)
    torch.manual_seed(0)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev).train()
    loss_fn = sel["loss"](cfg, comm)
    opt = ArenaAdam(ParamArena(mdl, adopt_conv=False), lr=1e-5)
    key = "evrel_seq_out" if row == "rob_evrel" else "evrel_seq_out_ones"
    assert (int(batch[key].numel() // batch[key].shape[-1]), int(batch[key].shape[-1])) == ROWS[row]
    direct, held = ops.gemm_bf16, {}
    via_copies = copies_gemm(held)

    def step():
        if arm == "bf16_copies":
            ops.gemm_bf16 = via_copies
        try:
            opt.zero_grad()
            loss = loss_fn(mdl(batch), batch)["loss"]
            loss.backward()
            opt.step()
        finally:
            ops.gemm_bf16 = direct
            held.clear()
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


def summary(per_round):
    med = {k: statistics.median(v) for k, v in per_round.items()}
    return {"ms_by_round": {k: [round(x, 5) for x in v] for k, v in per_round.items()},
            "median_ms": {k: round(v, 5) for k, v in med.items()},
            "round_to_round_spread_ms": {k: round(max(v) - min(v), 5) for k, v in per_round.items()}}


def backward_gemms(t, d, f):
    """[(kind, M, N, K, leading dimension of the strided A | None, uses per layer)] of one encoder layer's backward."""
    return [("dx attention.output.dense", t, d, d, None, 1), ("dx intermediate.dense", t, d, f, None, 1),
            ("dx output.dense", t, f, d, None, 1), ("dx fused q|k|v", t, d, 3 * d, None, 1),
            ("dW attention.output.dense", d, d, t, None, 1), ("dW query / key / value", d, d, t, 3 * d, 3),
            ("dW intermediate.dense", f, d, t, None, 1), ("dW output.dense", d, f, t, None, 1)]


def gemm_pair(kind, m, n, k, lda, dev, g, rounds, launches):
    from vidsitu_amd import ops

    if kind.startswith("dx"):  # dy [T, out] . W [out, in]: B strided
        dy, w = torch.randn(m, k, generator=g).to(dev), torch.randn(k, n, generator=g).to(dev)
        out = torch.empty(m, n, device=dev)
        fns = {"bf16_copies": lambda: ops.gemm_nt(dy, ops.transpose_f32(w), out=out, bf16=True),
               "bf16": lambda: ops.gemm_bf16(dy, w, out=out, b_t=True)}
    else:  # dy^T [out, T] . x [T, in]: both strided; with lda, dy is a column range of dqkv and is transposed whole
        dy_all, x = torch.randn(k, lda or m, generator=g).to(dev), torch.randn(k, n, generator=g).to(dev)
        outs = [torch.empty(m, n, device=dev) for _ in range((lda or m) // m)]

        def copies():
            dt, xt = ops.transpose_f32(dy_all), ops.transpose_f32(x)
            for s, o in enumerate(outs):
                ops.gemm_nt(dt[s * m:(s + 1) * m], xt, out=o, bf16=True)

        def strided():
            for s, o in enumerate(outs):
                ops.gemm_bf16(dy_all[:, s * m:(s + 1) * m], x, out=o, a_t=True, b_t=True)

        fns = {"bf16_copies": copies, "bf16": strided}
    for f in fns.values():
        f()
    res = summary(alternate(fns, rounds, launches))
    res["kind"], res["M_N_K"] = kind, [m, n, k]
    if lda:
        res["calls_per_figure"] = lda // m
    res["bf16_over_bf16_copies"] = round(res["median_ms"]["bf16"] / res["median_ms"]["bf16_copies"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roberta_matmul.json"))
    args = ap.parse_args()
    if args.rounds < 5 or args.steps < 5 or args.launches < 20:
        sys.exit("at least 5 rounds of at least 5 steps / 20 launches per arm")
    if not torch.cuda.is_available():
        sys.exit("roberta_matmul_bench.py measures on a GPU; none is visible")
    from vidsitu_amd.hf_roberta import ROBERTA_DIMS

    dev = torch.device("cuda:0")
    dims = ROBERTA_DIMS["roberta-base"]
    res = {"config": "RoBERTa-base, random weights, 8 videos, eager launches, forward + loss + backward + fused Adam; "
                     "arms: fp32 | bf16_copies (transpose_f32 + gemm_nt(bf16=True), this tool only) | bf16 (shipped)",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "steps_per_round": args.steps,
           "launches_per_round": args.launches,
           "unit": "ms per call, device events around a window of calls; arms alternate and rotate inside each round",
           "train_step": {}, "backward_gemms": {}}
    keep = True
    for row, (r, l) in ROWS.items():
        steps = {arm: build(row, arm, dev) for arm in ARMS}
        losses = {arm: round(float(steps[arm]().detach()), 6) for arm in ARMS}
        s = summary(alternate(steps, args.rounds, args.steps))
        med, spread = s["median_ms"], s["round_to_round_spread_ms"]
        s["sequences_x_tokens"], s["loss_after_three_steps"] = [r, l], losses
        s["fp32_over_bf16"] = round(med["fp32"] / med["bf16"], 4)
        s["fp32_over_bf16_copies"] = round(med["fp32"] / med["bf16_copies"], 4)
        s["bf16_copies_minus_bf16_ms"] = round(med["bf16_copies"] - med["bf16"], 5)
        s["strided_forms_pay_here"] = med["bf16_copies"] - med["bf16"] > spread["bf16_copies"]
        keep = keep and s["strided_forms_pay_here"]
        res["train_step"][row] = s
        print(row, json.dumps({k: v for k, v in s.items() if k != "ms_by_round"}))
        del steps
        torch.cuda.empty_cache()
    res["keep_strided_forms"] = keep
    res["keep_rule"] = "bf16_copies - bf16 (medians) > bf16_copies' round-to-round spread on both step shapes"
    g = torch.Generator().manual_seed(2)
    for row, (r, l) in ROWS.items():
        table, per_layer = [], {"bf16_copies": 0.0, "bf16": 0.0}
        for kind, m, n, k, lda, uses in backward_gemms(r * l, dims["d_model"], dims["d_ffn"]):
            e = gemm_pair(kind, m, n, k, lda, dev, g, args.rounds, args.launches)
            for a in per_layer:  # a figure with lda covers all its uses (the three weight gradients)
                per_layer[a] += e["median_ms"][a] * (1 if lda else uses)
            table.append(e)
            print(row, json.dumps({k2: v for k2, v in e.items() if k2 != "ms_by_round"}))
            torch.cuda.empty_cache()
        res["backward_gemms"][row] = {"tokens": r * l, "shapes": table,
                                      "per_layer_ms_from_the_table": {a: round(v, 4) for a, v in per_layer.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
