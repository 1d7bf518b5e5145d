#!/usr/bin/env python3
"""What bf16 weights buy caption generation: the `mdl.gpt2_decode_matmul=bf16` arm against the fp32 arm of the same run.

One process, two `sfpret_txe_txd_vbarg` models with a GPT-2 medium decoder (24 layers, d = 1024, vocabulary 50 259)
built from one state dict, one per mode.
  generation  2 videos x 5 events x beam 5 (50 rows), 60 tokens + the prompt (61 decode steps, min_len = max_len - 1 so
              that both arms run every step), device-side search.  Uses 1 and 2 of a search session run eagerly and
              capture the step graphs; timing starts at use 3, when every step is a graph replay (asserted).  `--rounds`
              rounds, the arms alternating and rotating who goes first, `--gens` generations per arm and round (the
              round's figure is their median), host wall clock around `EvalB_Gen.forward_one_batch`.
  gemms       the five GEMM shapes of a step alone, 50 rows, both forms, epilogues as the step has them.  One launch
              per weight image over a ring of distinct images of at least `--ring-mb` MiB (the 24 layers' images,
              cloned round-robin until the ring is that large; the lm_head's likewise): a loop over one weight -- or over
              24 bf16 ones, 151 MB -- would sit in the 256 MiB Infinity Cache and measure nothing a step sees.  The
              ring's launches are captured into one hipGraph (a step is replayed, too; eager launches of 5 us kernels
              would time the host) and timed by device events around a replay: us per launch, launch gaps included,
              and weight bytes per second.
Reported: per-round figures, medians, the fp32 arm's round-to-round spread (the noise a difference has to exceed), and
how many generated tokens differ between the arms on the same batch (informational).

    python tools/gpt2_decode_matmul_bench.py [--rounds 5] [--gens 3] [--out profiles/gpt2_decode_matmul.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("fp32", "bf16")
VIDEOS, EVENTS, BEAM, MAX_LEN = 2, 5, 5, 60
ROWS = VIDEOS * EVENTS * BEAM


def build(mode, dev, state_dict=None):
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    cfg = get_cfg({"task_type": "vb_arg", "mdl.mdl_name": "sfpret_txe_txd_vbarg", "mdl.tx_dec_type": "gpt2",
                   "mdl.gpt2_decode_matmul": mode, "gen.beam_size": BEAM, "gen.max_len_b": MAX_LEN,
                   "gen.min_len": MAX_LEN - 1})
    comm = synth_data.make_comm(cfg)
    sel = get_mdl_loss_eval(cfg)
    torch.manual_seed(0)
    mdl = sel["mdl"](cfg=cfg, comm=comm)
    if state_dict is not None:
        mdl.load_state_dict(state_dict)
    mdl = mdl.to(dev).eval()
    return cfg, comm, mdl, sel["evl"](cfg, comm, dev)


def session(mdl):
    (dec,) = [m for m in mdl.modules() if "_vs_search_sessions" in m.__dict__]
    return list(dec.__dict__["_vs_search_sessions"].values())[-1]


def generate(arm):
    _, _, mdl, evl, batch = arm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = evl.forward_one_batch(mdl, batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, [v["tokens"] for r in out for v in r["vb_output"].values()]


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v),
            "rounds": [round(x, 4) for x in v]}


def gemm_rings(gpt2s, dev, ring_mb):
    """{shape name: (n, k, {arm: (launch closure over the ring, images in the ring, bytes per image)})}."""
    from vidsitu_amd import ops

    d = gpt2s["fp32"].d_model
    vocab = gpt2s["fp32"].P("transformer.wte.weight").shape[0]
    n_layer = gpt2s["fp32"].n_layer
    g = torch.Generator().manual_seed(5)
    shapes = {"attn.c_attn": (3 * d, d, "attn.c_attn", dict(act=ops.ACT_NONE, res=False, ypk=False)),
              "attn.c_proj": (d, d, "attn.c_proj", dict(act=ops.ACT_NONE, res=True, ypk=False)),
              "mlp.c_fc": (4 * d, d, "mlp.c_fc", dict(act=ops.ACT_GELU_NEW, res=False, ypk=True)),
              "mlp.c_proj": (d, 4 * d, "mlp.c_proj", dict(act=ops.ACT_NONE, res=True, ypk=False)),
              "lm_head": (vocab, d, None, dict(act=ops.ACT_NONE, res=False, ypk=False))}
    rings = {}
    for name, (n, k, key, ep) in shapes.items():
        x = ops.pack_rows_f32((torch.randn(ROWS, k, generator=g)).to(dev))
        res = torch.randn(ROWS, n, generator=g).to(dev) if ep["res"] else None
        arms = {}
        for arm, m in gpt2s.items():
            fp32 = arm == "fp32"
            if key is None:
                srcs = [m.P("transformer.wte.weight").detach()]
                bias = None
            else:
                srcs = [m.P(f"transformer.h.{i}.{key}.weight").detach().t() for i in range(n_layer)]
                bias = m.P(f"transformer.h.0.{key}.bias")
            pack = ops.pack_rows_f32 if fp32 else ops.pack_rows_bf16
            imgs = [pack(s) for s in srcs]
            per = imgs[0].numel() * imgs[0].element_size()
            while len(imgs) * per < ring_mb * 2 ** 20:
                imgs.append(imgs[len(imgs) % len(srcs)].clone())
            gemm = ops.gemm_nt_packed if fp32 else ops.gemm_nt_packed_bf16

            def ring(imgs=imgs, gemm=gemm, x=x, n=n, k=k, bias=bias, res=res, ep=ep):
                for w in imgs:
                    gemm(x, w, ROWS, n, k, b=bias, res=res, act=ep["act"], y_packed=ep["ypk"])

            arms[arm] = (ring, len(imgs), per)
        rings[name] = (n, k, arms)
    return rings


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gens", type=int, default=3)
    ap.add_argument("--ring-mb", type=int, default=512)
    ap.add_argument("--commit", default=None, help="recorded in the JSON (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpt2_decode_matmul.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpt2_decode_matmul_bench.py measures on a GPU; none is visible")
    if args.rounds < 5:
        sys.exit("at least 5 rounds")
    from vidsitu_amd import synth_data
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip

    dev = torch.device("cuda:0")
    commit = args.commit
    if commit is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"

    arms, sd = {}, None
    for mode in ARMS:
        cfg, comm, mdl, evl = build(mode, dev, sd)
        if sd is None:
            sd = {k: v.detach().cpu().clone() for k, v in mdl.state_dict().items()}
        batch = synth_data.synth_srl_batch(comm, bs=VIDEOS, n_ev=EVENTS, seq_len=60, device=dev)
        arms[mode] = (cfg, comm, mdl, evl, batch)
    gpt2s = {a: [m for m in arms[a][2].modules() if isinstance(m, GPT2LMHeadModelHip)][0] for a in ARMS}
    assert [gpt2s[a].decode_matmul for a in ARMS] == list(ARMS)
    vocab = gpt2s["fp32"].P("transformer.wte.weight").shape[0]

    # ---- (a) one generation ---------------------------------------------------------------------------------------
    tokens = {}
    for a in ARMS:  # use 1 eager, use 2 captures the step graphs
        for use in (1, 2):
            _, tokens[a] = generate(arms[a])
            assert session(arms[a][2]).uses == use
    per_round = {a: [] for a in ARMS}
    for rnd in range(args.rounds):
        order = ARMS[rnd % 2:] + ARMS[:rnd % 2]
        for a in order:
            ms = []
            for _ in range(args.gens):
                dt, toks = generate(arms[a])
                ses = session(arms[a][2])
                assert ses.uses >= 3 and len(ses.graphs) > 0 and toks == tokens[a], (a, ses.uses)
                ms.append(dt)
            per_round[a].append(statistics.median(ms))
    steps = MAX_LEN + 1
    n_tok = sum(len(t) for t in tokens["fp32"])
    differ = sum(sum(1 for x, y in zip(p, q) if x != y) + abs(len(p) - len(q))
                 for p, q in zip(tokens["fp32"], tokens["bf16"]))
    gen = {a: summary(per_round[a]) for a in ARMS}
    for a in ARMS:
        gen[a]["median_ms_per_step"] = gen[a]["median"] / steps

    # ---- (b) the five GEMM shapes alone ---------------------------------------------------------------------------
    gemms = {}
    for name, (n, k, by_arm) in gemm_rings(gpt2s, dev, args.ring_mb).items():
        graphs = {}
        for a, (ring, count, per) in by_arm.items():
            ring()  # warm-up: first-use attributes, allocator
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                ring()
            g.replay()
            torch.cuda.synchronize()
            graphs[a] = (g, count, per)
        us = {a: [] for a in ARMS}
        for rnd in range(args.rounds):
            order = ARMS[rnd % 2:] + ARMS[:rnd % 2]
            for a in order:
                g, count, _ = graphs[a]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                torch.cuda.synchronize()
                us[a].append(e0.elapsed_time(e1) * 1e3 / count)
        row = {"M": ROWS, "N": n, "K": k}
        for a in ARMS:
            _, count, per = graphs[a]
            s = summary(us[a])
            row[a] = {"us_per_launch": s, "images_in_ring": count, "weight_bytes": per,
                      "weight_GB_per_s": per / s["median"] * 1e-3}
        row["bf16_over_fp32_time"] = row["bf16"]["us_per_launch"]["median"] / row["fp32"]["us_per_launch"]["median"]
        gemms[name] = row
        del graphs

    res = {"commit": commit, "device": torch.cuda.get_device_name(0),
           "shape": {"decoder": "gpt2-medium", "vocab": vocab, "videos": VIDEOS, "events": EVENTS, "beam": BEAM,
                     "rows": ROWS, "decode_steps": steps, "device_search": True, "timed_from_use": 3,
                     "rounds": args.rounds, "generations_per_round": args.gens, "ring_MiB_at_least": args.ring_mb},
           "timed": {"generation": "host wall clock around EvalB_Gen.forward_one_batch, every step a hipGraph replay; "
                                   "a round's figure is the median of its generations",
                     "gemms": "device events around one replay of a hipGraph holding one launch per image of the ring; "
                              "us per launch includes the gaps between graph nodes"},
           "generation_ms": gen,
           "generation_bf16_minus_fp32_median_ms": gen["bf16"]["median"] - gen["fp32"]["median"],
           "generation_bf16_over_fp32": gen["bf16"]["median"] / gen["fp32"]["median"],
           "bf16_faster_by_more_than_the_fp32_spread":
               gen["fp32"]["median"] - gen["bf16"]["median"] > gen["fp32"]["spread"],
           "generated_tokens": {"of_the_fp32_arm": n_tok, "differing_between_the_arms": differ,
                                "captions_differing": sum(p != q for p, q in zip(tokens["fp32"], tokens["bf16"])),
                                "captions": len(tokens["fp32"])},
           "gemm_shapes": gemms}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for a in ARMS:
        s = gen[a]
        print(f"generation {a}: median {s['median']:.2f} ms ({s['median_ms_per_step']:.3f} ms / step), "
              f"rounds {s['min']:.2f} .. {s['max']:.2f}")
    print(f"tokens differing between the arms: {differ} of {n_tok}")
    for name, row in gemms.items():
        print(f"{name} {ROWS} x {row['N']} x {row['K']}: " + ", ".join(
            f"{a} {row[a]['us_per_launch']['median']:.2f} us ({row[a]['weight_GB_per_s']:.0f} GB/s)" for a in ARMS))


if __name__ == "__main__":
    main()
