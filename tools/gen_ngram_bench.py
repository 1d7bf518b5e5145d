"""What n-gram blocking costs a generation (`gen.no_repeat_ngram_size`): the shape of tools/gpt2_gen_bench.py
(B videos x 5 events, beam 5, 60 tokens, device-side search, GPT-2-medium decoder or `DEC=txdec`) with
n = 0 and n = 3 alternating in one process.  Each arm has its own search session; timing starts at the third
use of each, when every step is a graph replay.  The ban lives inside the scoring kernel, so the claim to
check is: same launches per generation, n = 3 within the run-to-run spread of the n = 0 arm.
Writes medians and spreads to profiles/gen_ngram.json (or `--out PATH`).  Informational, not bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vidsitu_amd import _lib, synth_data
from vidsitu_amd.extended_config import get_cfg
from vidsitu_amd.mdl_selector import get_mdl_loss_eval

ap = argparse.ArgumentParser()
ap.add_argument("--videos", type=int, default=2)
ap.add_argument("--beam", type=int, default=5)
ap.add_argument("--max-len", type=int, default=60)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              "profiles", "gen_ngram.json"))
args = ap.parse_args()

dev = torch.device("cuda:0")
dec = os.environ.get("DEC", "gpt2")
cfg = get_cfg({"task_type": "vb_arg", "mdl.mdl_name": "sfpret_txe_txd_vbarg", "mdl.tx_dec_type": dec,
               "gen.beam_size": args.beam, "gen.max_len_b": args.max_len, "gen.min_len": args.max_len - 1})
comm = synth_data.make_comm(cfg)
sel = get_mdl_loss_eval(cfg)
torch.manual_seed(0)
mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev).eval()
batch = synth_data.synth_srl_batch(comm, bs=args.videos, n_ev=5, seq_len=60, device=dev)
evl = sel["evl"](cfg, comm, dev)
lib = _lib.load()
ARMS = (0, 3)


def generate(n):
    evl.cfg.gen.no_repeat_ngram_size = n
    torch.cuda.synchronize()
    c0, t0 = lib.vs_launch_count(), time.perf_counter()
    out = evl.forward_one_batch(mdl, batch)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt * 1e3, lib.vs_launch_count() - c0, [v["tokens"] for r in out for v in r["vb_output"].values()]


def repeats(seqs, n):
    pad = comm.gpt2_hf_tok.pad_token_id
    bad = 0
    for s in seqs:
        s = [comm.gpt2_hf_tok.eos_token_id] + [t for t in s if t != pad]
        grams = [tuple(s[i: i + n]) for i in range(len(s) - n + 1)]
        bad += len(grams) != len(set(grams))
    return bad


warm = {n: [generate(n) for _ in range(2)] for n in ARMS}  # use 1 eager, use 2 captures the step graphs
ms = {n: [] for n in ARMS}
tokens = {}
for _ in range(args.reps):
    for n in ARMS:
        dt, _, tokens[n] = generate(n)
        ms[n].append(dt)


def summary(v):
    q = statistics.quantiles(v, n=4)
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "iqr_ms": q[2] - q[0],
            "spread_ms": max(v) - min(v), "samples_ms": [round(x, 3) for x in v]}


res = {"shape": {"videos": args.videos, "events": 5, "beam": args.beam, "max_len": args.max_len, "decoder": dec,
                 "device_search": True, "reps_per_arm": args.reps, "timed_from_use": 3},
       "n0": summary(ms[0]), "n3": summary(ms[3]),
       "n3_minus_n0_median_ms": statistics.median(ms[3]) - statistics.median(ms[0]),
       "n3_median_within_n0_spread": min(ms[0]) <= statistics.median(ms[3]) <= max(ms[0]),
       # host-side launches of a whole generation.  Use 2 (every step is launched once, into its graph) is the
       # like-for-like pair; use 1 of the n = 0 arm is the first generation of the process and also holds
       # its one-time launches
       "launches_use1_eager": {"n0": warm[0][0][1], "n3": warm[3][0][1]},
       "launches_use2_capture": {"n0": warm[0][1][1], "n3": warm[3][1][1]},
       "sequences_with_a_repeated_trigram": {"n0": repeats(tokens[0], 3), "n3": repeats(tokens[3], 3)},
       "device": torch.cuda.get_device_name(0)}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps({k: v for k, v in res.items() if k not in ("n0", "n3")}))
for n in ARMS:
    s = res[f"n{n}"]
    print(f"n = {n}: median {s['median_ms']:.2f} ms, min {s['min_ms']:.2f}, max {s['max_ms']:.2f}, iqr {s['iqr_ms']:.2f}")
