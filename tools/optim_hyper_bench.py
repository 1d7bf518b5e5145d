#!/usr/bin/env python3
"""What the device-side hyper-parameters of `ArenaAdam` cost per step, at the bench step's own configuration
(SlowFast-R50 + 6-layer TxEncoder, 8 clips as 2 videos x 4 events, bf16, whole-step hipGraph, grad_fill="learn").

Three `TrainStep`s, each on its own model built from one seed, are replayed in alternating rounds in ONE process:
  (a) default `ArenaAdam`                      -- the rate is a launch argument (what bench.py measures)
  (b) `dynamic_lr=True`                        -- same bytes, the rate read from device memory
  (c) `dynamic_lr` + `max_grad_norm` + `weight_decay` -- one more read of the gradient arena (the norm pass)
Each round times `--replays` replays per arm between two device events.  Reported: the median over rounds per arm,
the per-round spread of (a) against itself (the noise a difference has to exceed), the norm kernel's and the Adam
kernel's own time (device events around `--replays` launches each), and the bytes each moves over that time.

    python tools/optim_hyper_bench.py [--rounds 5] [--replays 50] [--out profiles/optim_hyper.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = {
    "a_default": {},
    "b_dynamic_lr": {"dynamic_lr": True},
    "c_dynamic_lr_clip_wd": {"dynamic_lr": True, "max_grad_norm": 1.0, "weight_decay": 0.01},
}


def build(kw, dev):
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval
    from vidsitu_amd.optim import ArenaAdam, ParamArena
    from vidsitu_amd.train_step import TrainStep

    cfg = get_cfg({"mdl.mdl_name": "sf_base_txenc", "tx_dec.encoder_layers": 6})
    comm = synth_data.make_comm(cfg)
    torch.manual_seed(0)
    sel = get_mdl_loss_eval(cfg)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev).train()
    batch = synth_data.synth_batch(cfg, comm, bs=2, n_ev=4, seed=1234, device=dev, dtype=torch.bfloat16)
    arena = ParamArena(mdl)
    opt = ArenaAdam(arena, lr=cfg.train.lr, betas=(0.9, 0.99), **kw)
    ts = TrainStep(mdl, sel["loss"](cfg, comm), arena, opt, batch, world=1, use_dist=False, grad_fill="learn")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ts.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ts.capture()
    for _ in range(3):  # the first launch uploads the graph
        ts.replay()
    torch.cuda.synchronize()
    return ts


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--out", default="profiles/optim_hyper.json")
    args = ap.parse_args()
    if args.rounds < 5 or args.replays < 50:
        sys.exit("at least 5 rounds of at least 50 replays per arm")
    if not torch.cuda.is_available():
        sys.exit("optim_hyper_bench.py measures on a GPU; none is visible")
    from vidsitu_amd import ops

    dev = torch.device("cuda:0")
    steps = {name: build(kw, dev) for name, kw in ARMS.items()}
    per_round = {name: [] for name in ARMS}
    names = list(ARMS)
    for r in range(args.rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:  # rotate who goes first
            per_round[name].append(timed(steps[name].replay, args.replays))
    med = {name: statistics.median(v) for name, v in per_round.items()}
    a = per_round["a_default"]
    spread_a = max(a) - min(a)

    # the two kernels on their own, on arm (c)'s arena (fp32 gradients: no process group)
    ts = steps["c_dynamic_lr_clip_wd"]
    opt, arena = ts.opt, ts.arena
    n = arena.numel
    norm_ms = timed(lambda: ops.grad_sumsq(arena.grad, opt.sumsq_ws), args.replays)
    adam_ms = timed(lambda: ops.adam_step_hp(arena.data, arena.grad, opt.m, opt.v, arena.data_bf16, opt.hyper,
                                             opt.betas[0], opt.betas[1], opt.eps, opt.t, tick=True,
                                             sumsq_ws=opt.sumsq_ws), args.replays)
    d = steps["a_default"]
    adam_default_ms = timed(lambda: ops.adam_step_dev_cast(d.arena.data, d.arena.grad, d.opt.m, d.opt.v,
                                                           d.arena.data_bf16, d.opt.lr, d.opt.betas[0], d.opt.betas[1],
                                                           d.opt.eps, d.opt.t), args.replays)
    adam_bytes = n * (4 * 4 + 3 * 4 + 2)  # reads p, g, m, v; writes p, m, v and the bf16 copy
    norm_bytes = n * 4
    adam_tbs = adam_bytes / (adam_ms * 1e-3) / 1e12
    res = {
        "config": "SlowFast-R50 + 6-layer TxEncoder, 8 clips (2 x 4), bf16, whole-step hipGraph, grad_fill=learn",
        "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "replays_per_round": args.replays,
        "arena_elements": n,
        "ms_per_step_by_round": {k: [round(x, 4) for x in v] for k, v in per_round.items()},
        "median_ms_per_step": {k: round(v, 4) for k, v in med.items()},
        "a_round_to_round_spread_ms": round(spread_a, 4),
        "b_minus_a_ms": round(med["b_dynamic_lr"] - med["a_default"], 4),
        "b_within_a_spread": abs(med["b_dynamic_lr"] - med["a_default"]) <= spread_a,
        "c_minus_a_ms": round(med["c_dynamic_lr_clip_wd"] - med["a_default"], 4),
        "norm_kernel_ms": round(norm_ms, 4), "norm_kernel_bytes": norm_bytes,
        "norm_kernel_TBps": round(norm_bytes / (norm_ms * 1e-3) / 1e12, 3),
        "adam_hp_kernel_ms": round(adam_ms, 4), "adam_default_kernel_ms": round(adam_default_ms, 4),
        "adam_kernel_bytes": adam_bytes, "adam_hp_kernel_TBps": round(adam_tbs, 3),
        "norm_pass_ms_at_adam_bandwidth": round(norm_bytes / (adam_tbs * 1e12) * 1e3, 4),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
