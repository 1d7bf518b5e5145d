#!/usr/bin/env python3
"""The key-tiled attention family (csrc/attn_tiled.hip) beside the LDS-resident kernels -> profiles/attn_tiled.json.

  python tools/attn_tiled_bench.py [--rounds 7] [--iters 20] [--out profiles/attn_tiled.json]

Four shapes at dh = 64: the two the models run today (both families hold them; ops.py keeps them on the resident
kernels) and two only the tiled family holds -- a roberta-base batch at 512 tokens, a gpt2 batch at 1024.  Forward and
backward, without dropout, right padding of differing lengths.  The tiled kernels are called through their own entry
points, the resident ones through theirs, so in-range shapes measure both.

Method (tools/evrel_bench.py): every timed window is a run of `iters` calls between two device events after a
synchronise; the arms alternate inside each round; median and minimum over the rounds.  Two warm-up calls per arm come
first.  TFLOP/s counts 2 * dh flops per (query, key) pair and product -- two products forward (QK^T, PV), five backward
(QK^T, dO V^T, dS K, P^T dO, dS^T Q; the tiled backward computes the first two twice in launch A and once more in
launch B, which is not counted) -- over L * L pairs under the padding rule and L * (L + 1) / 2 under the causal rule.
The numbers gate nothing.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("pad", 32, 120, 12, 64), ("pad", 32, 512, 12, 64), ("causal", 50, 60, 16, 64), ("causal", 8, 1024, 16, 64)]


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
    for fn in variants.values():
        fn()
        fn()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, iters))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                "rounds_ms": [round(x, 4) for x in v]} for k, v in ms.items()}


def measure(rule, r, l, h, dh, dev, rounds, iters):
    from vidsitu_amd import ops

    causal = rule == "causal"
    lib = ops._lib.load()
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(r * l, 3 * h * dh, generator=g).to(dev)
    dout = torch.randn(r * l, h * dh, generator=g).to(dev)
    mask = torch.ones(r, l, dtype=torch.uint8)
    for i in range(r):  # right padding of differing lengths, up to half the sequence
        mask[i, l - (i * 7) % (l // 2):] = 0
    mask = mask.to(dev)
    out, dqkv = torch.empty(r * l, h * dh, device=dev), torch.empty_like(qkv)
    ws = ops._workspace(lib.vs_attn_tiled_bwd_scratch_bytes(r, l, h), dev)

    def tiled_fwd():
        ops._lib.call("vs_attn_tiled_fwd", ops._ptr(qkv), ops._ptr(mask), ops._ptr(out), r, l, h, dh, int(causal), None,
                      0, 0, 1.0, ops._stream())

    def tiled_bwd():
        ops._lib.call("vs_attn_tiled_bwd", ops._ptr(qkv), ops._ptr(mask), ops._ptr(dout), ops._ptr(dqkv), ops._ptr(ws),
                      ws.numel(), r, l, h, dh, int(causal), None, 0, 0, 1.0, ops._stream())

    arms = {"tiled_fwd": tiled_fwd, "tiled_bwd": tiled_bwd}
    fits = {k: bool(lib.vs_attn_resident_fits(int(causal), l, dh, b)) for k, b in (("fwd", 0), ("bwd", 1))}
    fwd, bwd = (ops.attn_causal, ops.attn_causal_bwd) if causal else (ops.attn_pad, ops.attn_pad_bwd)
    if fits["fwd"]:  # (ops.py sends exactly these to the resident kernels)
        arms["resident_fwd"] = lambda: fwd(qkv, mask, r, l, h)
    if fits["bwd"]:
        arms["resident_bwd"] = lambda: bwd(qkv, mask, dout, r, l, h)
    res = alternate(arms, rounds, iters)
    pairs = r * h * (l * (l + 1) // 2 if causal else l * l)
    for k, v in res.items():
        flop = pairs * dh * 2 * (2 if k.endswith("fwd") else 5)
        v["tflops_median"] = round(flop / v["median_ms"] / 1e9, 2)
    for k in ("fwd", "bwd"):
        if fits[k]:
            res[f"tiled_over_resident_{k}_median"] = round(res[f"tiled_{k}"]["median_ms"]
                                                           / res[f"resident_{k}"]["median_ms"], 3)
    res["shape"] = {"rule": rule, "R": r, "L": l, "H": h, "dh": dh}
    res["resident_holds"] = fits
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_tiled.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_tiled_bench.py measures on the GPU only")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters_per_window": a.iters,
           "unit": "ms per call, device events around a window of calls; arms alternate inside each round",
           "beside": "resident pad kernel: 24-27 TFLOP/s (profiles/evrel_step.json)", "shapes": []}
    for shape in SHAPES:
        out["shapes"].append(measure(*shape, dev, a.rounds, a.iters))
        print(json.dumps({k: (v if not isinstance(v, dict) or "rounds_ms" not in v
                              else {x: y for x, y in v.items() if x != "rounds_ms"})
                          for k, v in out["shapes"][-1].items()}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
