#!/usr/bin/env python3
"""Event-relation training step and the padding-masked attention kernels, measured -> profiles/evrel_step.json.

  python tools/evrel_bench.py [--rounds 7] [--iters 5] [--out profiles/evrel_step.json]

1. ms per training step (forward + backward + Adam) at roberta-base dimensions with random weights and 8 videos, for
   `sfpret_evrel` (40 sequences x 60 tokens) and `rob_evrel` (32 x 120): this package's model on ArenaAdam, alternated
   round by round in ONE process with the plain-torch restatement (tests/roberta_ref.py, fp32 on the same GPU through
   PyTorch-ROCm, torch.optim.Adam).  Both start from the same weights and see the same batch; the first loss of each
   is recorded so that the two can be seen to compute the same thing.
2. vs_attn_pad_fwd / _bwd against vs_attn_causal_fwd / _bwd at the same R, L, H, dh.  The causal kernels do half the
   (query, key) pairs, on the vector units: the only in-tree yardstick for what the matrix path buys.

Method: every timed window is a run of `iters` calls between two device events after a synchronise; the variants
alternate inside each round; median and minimum over the rounds are reported.  Two warm-up calls per variant come first
(code objects, allocator, the encoder's fused-weight cache).  The numbers gate nothing.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(variants, rounds, iters):
    """{name: fn} -> {name: {"median_ms", "min_ms", "rounds_ms"}}, the variants alternating inside every round."""
    for fn in variants.values():
        fn()
        fn()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, iters))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                "rounds_ms": [round(x, 4) for x in v]} for k, v in ms.items()}


def step_pair(row, dev, rounds, iters):
    import roberta_ref as ref
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.hf_roberta import ROBERTA_DIMS
    from vidsitu_amd.mdl_sf_base import get_head_dim
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval
    from vidsitu_amd.optim import ArenaAdam, ParamArena

    cfg = get_cfg({"task_type": "evrel", "mdl.mdl_name": row, "mdl.rob_mdl_name": "roberta-base"})
    comm = synth_data.make_comm(cfg)
    dims = ROBERTA_DIMS["roberta-base"]
    batch = synth_data.synth_evrel_batch(comm, 8, n_ann=1, feat_dim=get_head_dim(cfg), seed=7, device=dev)
    sel = get_mdl_loss_eval(cfg)
    torch.manual_seed(0)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev).train()
    # the restatement starts from a copy of the same weights (taken before the arena adopts the parameters)
    w = {k: v.detach().clone().requires_grad_(True) for k, v in mdl.state_dict().items()}
    loss_fn = sel["loss"](cfg, comm)
    opt = ArenaAdam(ParamArena(mdl, adopt_conv=False), lr=1e-5)
    topt = torch.optim.Adam(list(w.values()), lr=1e-5, betas=(0.9, 0.99))
    first = {}

    def hip_step():
        opt.zero_grad()
        loss = loss_fn(mdl(batch), batch)["loss"]
        loss.backward()
        opt.step()
        first.setdefault("hip", loss.detach())

    def torch_step():
        topt.zero_grad(set_to_none=True)
        _, loss = ref.evrel_forward(row, w, batch, dims)
        loss.backward()
        topt.step()
        first.setdefault("torch", loss.detach())

    res = alternate({"hip": hip_step, "torch": torch_step}, rounds, iters)
    key = "evrel_seq_out" if row == "rob_evrel" else "evrel_seq_out_ones"
    res["sequences_x_tokens"] = [int(batch[key].numel() // batch[key].shape[-1]), int(batch[key].shape[-1])]
    res["first_loss"] = {k: round(float(v), 6) for k, v in first.items()}
    res["torch_over_hip_median"] = round(res["torch"]["median_ms"] / res["hip"]["median_ms"], 3)
    return res


def attn_pair(r, l, h, dh, dev, rounds, iters):
    from vidsitu_amd import ops

    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(r * l, 3 * h * dh, generator=g).to(dev)
    dout = torch.randn(r * l, h * dh, generator=g).to(dev)
    mask = torch.ones(r, l, dtype=torch.uint8)
    for i in range(r):  # right padding of differing lengths, up to half the sequence
        mask[i, l - (i * 7) % (l // 2):] = 0
    mask = mask.to(dev)
    res = alternate({"attn_pad_fwd": lambda: ops.attn_pad(qkv, mask, r, l, h),
                     "attn_causal_fwd": lambda: ops.attn_causal(qkv, mask, r, l, h),
                     "attn_pad_bwd": lambda: ops.attn_pad_bwd(qkv, mask, dout, r, l, h),
                     "attn_causal_bwd": lambda: ops.attn_causal_bwd(qkv, mask, dout, r, l, h)}, rounds, iters * 10)
    pairs = r * h * l * l  # (query, key) pairs the bidirectional kernel scores; the causal one does half
    for k in ("fwd", "bwd"):
        flop = pairs * dh * 2 * (2 if k == "fwd" else 5)  # QK^T, PV | QK^T, dO V^T, dS K, P^T dO, dS^T Q
        res[f"attn_pad_{k}"]["gflops_median"] = round(flop / res[f"attn_pad_{k}"]["median_ms"] / 1e6, 1)
        res[f"causal_over_pad_{k}_median"] = round(res[f"attn_causal_{k}"]["median_ms"]
                                                   / res[f"attn_pad_{k}"]["median_ms"], 3)
    res["shape"] = {"R": r, "L": l, "H": h, "dh": dh}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evrel_step.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("evrel_bench.py measures on the GPU only")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters_per_window": a.iters,
           "unit": "ms per call, device events around a window of calls; variants alternate inside each round",
           "train_step": {}, "attention": []}
    for row in ("sfpret_evrel", "rob_evrel"):
        out["train_step"][row] = step_pair(row, dev, a.rounds, a.iters)
        print(row, json.dumps({k: v for k, v in out["train_step"][row].items() if k != "rounds_ms"}))
        torch.cuda.empty_cache()
    for r, l in ((40, 60), (32, 120)):
        out["attention"].append(attn_pair(r, l, 12, 64, dev, a.rounds, a.iters))
        print("attention", json.dumps(out["attention"][-1]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
