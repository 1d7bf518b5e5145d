#!/usr/bin/env python3
"""Encoder attention over source sequences (csrc/attn_cross.hip) and the `txed_only` row -> profiles/txdec_cross.json.

  python tools/txdec_cross_bench.py [--rounds 5] [--iters 20] [--parent DIR] [--out profiles/txdec_cross.json]

Four measurements:
  kernels   attn_cross forward and backward at R 40, L 60, H 8, dh 128, S in {5, 60}, right padding of differing
            lengths, beside torch's own fp32 attention (scaled_dot_product_attention and its autograd) with the same
            mask on the same device.
  decode    the one-query decode kernel beside the general forward kernel at L = 1, rows 50, S in {5, 60}.
  txed_only the row's training step and one generation (beam 5) at mdl.txed_src prompt and vb.
  sfpret    the `sfpret_txe_txd_vbarg` training step and generation (the S = 1 path) in this tree and, with --parent
            DIR (a built checkout of the parent commit), in that one: fresh child processes, alternating, one pair per
            round; the parent arm's own round-to-round spread is recorded beside the difference.

Method (tools/attn_tiled_bench.py): every timed window is a run of `iters` calls between two device events after a
synchronise; the arms alternate inside each round; median, minimum and spread (max - min) over the rounds.  Two warm-up
calls per arm come first.  The numbers gate nothing.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
            "spread_ms": round(max(v) - min(v), 4), "rounds_ms": [round(x, 4) for x in v]}


def alternate(variants, rounds, iters):
    for fn in variants.values():
        fn()
        fn()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, iters))
    return {k: summary(v) for k, v in ms.items()}


def _mask(r, s, dev):
    m = torch.ones(r, s, dtype=torch.uint8)
    for i in range(r):  # right padding of differing lengths, at least one valid key
        m[i, s - (i * 7) % s:] = 0 if (i * 7) % s else 1
    return m.to(dev)


def kernels(r, l, s, h, dh, dev, rounds, iters):
    import torch.nn.functional as F
    from vidsitu_amd import ops

    g = torch.Generator().manual_seed(3)
    d = h * dh
    q, kv = torch.randn(r * l, d, generator=g).to(dev), torch.randn(r * s, 2 * d, generator=g).to(dev)
    dout = torch.randn(r * l, d, generator=g).to(dev)
    mask = _mask(r, s, dev)
    q4 = q.view(r, l, h, dh).transpose(1, 2).contiguous().requires_grad_(True)
    k4 = kv[:, :d].reshape(r, s, h, dh).transpose(1, 2).contiguous().requires_grad_(True)
    v4 = kv[:, d:].reshape(r, s, h, dh).transpose(1, 2).contiguous().requires_grad_(True)
    do4 = dout.view(r, l, h, dh).transpose(1, 2).contiguous()
    am = mask.bool()[:, None, None, :]

    def torch_fwd():
        with torch.no_grad():
            F.scaled_dot_product_attention(q4, k4, v4, attn_mask=am)

    def torch_fwd_bwd():
        o = F.scaled_dot_product_attention(q4, k4, v4, attn_mask=am)
        torch.autograd.grad(o, (q4, k4, v4), do4)

    res = alternate({"attn_cross_fwd": lambda: ops.attn_cross(q, kv, mask, r, l, s, h),
                     "attn_cross_bwd": lambda: ops.attn_cross_bwd(q, kv, mask, dout, r, l, s, h),
                     "torch_fwd": torch_fwd, "torch_fwd_bwd": torch_fwd_bwd}, rounds, iters)
    res["torch_bwd_median_ms"] = round(res["torch_fwd_bwd"]["median_ms"] - res["torch_fwd"]["median_ms"], 4)
    res["fwd_over_torch_median"] = round(res["attn_cross_fwd"]["median_ms"] / res["torch_fwd"]["median_ms"], 3)
    res["bwd_over_torch_median"] = round(res["attn_cross_bwd"]["median_ms"] / max(res["torch_bwd_median_ms"], 1e-6), 3)
    res["shape"] = {"R": r, "L": l, "S": s, "H": h, "dh": dh}
    return res


def decode(rows, s, h, dh, dev, rounds, iters):
    from vidsitu_amd import ops

    g = torch.Generator().manual_seed(4)
    d = h * dh
    q, kv = torch.randn(rows, d, generator=g).to(dev), torch.randn(rows * s, 2 * d, generator=g).to(dev)
    mask = _mask(rows, s, dev)
    kc, vc = torch.empty(rows, h, s, dh, device=dev), torch.empty(rows, h, s, dh, device=dev)
    ops.attn_cross_kv_split(kv, kc, vc)
    res = alternate({"decode_kernel": lambda: ops.attn_cross_decode(q, kc, vc, mask),
                     "forward_kernel_L1": lambda: ops.attn_cross(q, kv, mask, rows, 1, s, h)}, rounds, iters)
    res["decode_over_forward_median"] = round(res["decode_kernel"]["median_ms"]
                                              / res["forward_kernel_L1"]["median_ms"], 3)
    res["shape"] = {"rows": rows, "S": s, "H": h, "dh": dh}
    return res


def _row(over, dev):
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_sf_base import get_head_dim
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval
    from vidsitu_amd.optim import ArenaAdam, ParamArena
    from vidsitu_amd.seq_gen import SeqGenCustom

    cfg = get_cfg(dict({"task_type": "vb_arg", "mdl.tx_dec_type": "txdec", "gen.beam_size": 5}, **over))
    comm = synth_data.make_comm(cfg)
    sel = get_mdl_loss_eval(cfg)
    torch.manual_seed(0)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev)
    batch = synth_data.synth_srl_batch(comm, 8, 5, feat_dim=get_head_dim(cfg), seq_len=60, device=dev)
    opt = ArenaAdam(ParamArena(mdl, adopt_conv=False), lr=1e-5)
    loss_fn = sel["loss"](cfg, comm)

    def step():
        mdl.train()
        opt.zero_grad()
        loss_fn(mdl(batch), batch)["loss"].backward()
        opt.step()

    def generate():
        mdl.eval()
        gen = SeqGenCustom([mdl], tgt_dict=comm.gpt2_hf_tok, **{k: cfg.gen[k] for k in cfg.gen})
        with torch.no_grad():
            mdl.forward_gen(dict(batch), gen)

    return step, generate


def txed_only(dev, rounds):
    arms = {}
    for src in ("prompt", "vb"):
        step, gen = _row({"mdl.mdl_name": "txed_only", "mdl.tx_enc_type": "old", "mdl.txed_src": src}, dev)
        arms[f"train_step_{src}"], arms[f"generate_{src}"] = step, gen
    gens = {k: v for k, v in arms.items() if k.startswith("generate")}
    for fn in gens.values():
        fn()  # the third use of a shape replays its captured steps
    res = alternate({k: v for k, v in arms.items() if k.startswith("train")}, rounds, 5)
    res.update(alternate(gens, rounds, 1))
    res["shape"] = {"rows": 40, "L": 60, "beam": 5}
    return res


def sfpret_once(dev):
    """One child's worth of the S = 1 row: medians over 3 windows, printed as one JSON line."""
    step, gen = _row({"mdl.mdl_name": "sfpret_txe_txd_vbarg"}, dev)
    for _ in range(2):
        step()
    for _ in range(3):
        gen()
    out = {"train_step_ms": statistics.median(timed(step, 5) for _ in range(3)),
           "generate_ms": statistics.median(timed(gen, 1) for _ in range(3))}
    print("SFPRET " + json.dumps(out))


def sfpret(parent, rounds):
    trees = {"this": ROOT}
    if parent:
        trees["parent"] = os.path.abspath(parent)
    ms = {k: {"train_step_ms": [], "generate_ms": []} for k in trees}
    for _ in range(rounds):
        for k, root in trees.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sfpret-child", "--tree", root],
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"{k} arm failed: {r.stdout[-2000:]}{r.stderr[-2000:]}")
            line = [x for x in r.stdout.splitlines() if x.startswith("SFPRET ")][-1]
            for key, v in json.loads(line[7:]).items():
                ms[k][key].append(v)
    res = {k: {key: summary(v) for key, v in d.items()} for k, d in ms.items()}
    if parent:
        for key in ("train_step_ms", "generate_ms"):
            res[f"this_minus_parent_{key}_median"] = round(res["this"][key]["median_ms"]
                                                           - res["parent"][key]["median_ms"], 4)
            res[f"parent_spread_{key}"] = res["parent"][key]["spread_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "txdec_cross.json"))
    ap.add_argument("--sfpret-child", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    if not torch.cuda.is_available():
        sys.exit("txdec_cross_bench.py measures on the GPU only")
    dev = torch.device("cuda:0")
    if a.sfpret_child:
        return sfpret_once(dev)
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters_per_window": a.iters,
           "unit": "ms per call, device events around a window of calls; arms alternate inside each round",
           "kernels": [], "decode": []}

    def show(tag, res):
        print(tag, json.dumps({k: (v if not isinstance(v, dict) or "rounds_ms" not in v
                                   else {x: y for x, y in v.items() if x != "rounds_ms"}) for k, v in res.items()}))

    for s in (5, 60):
        out["kernels"].append(kernels(40, 60, s, 8, 128, dev, a.rounds, a.iters))
        show("kernels", out["kernels"][-1])
    for s in (5, 60):
        out["decode"].append(decode(50, s, 8, 128, dev, a.rounds, a.iters))
        show("decode", out["decode"][-1])
    out["txed_only"] = txed_only(dev, a.rounds)
    show("txed_only", out["txed_only"])
    out["sfpret_txe_txd_vbarg"] = sfpret(a.parent, a.rounds)
    print("sfpret", json.dumps({k: v for k, v in out["sfpret_txe_txd_vbarg"].items() if not isinstance(v, dict)}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
