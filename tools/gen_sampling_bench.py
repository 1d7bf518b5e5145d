"""What a sampling search costs a generation (`gen.sampling`, `gen.sampling_topk`, `gen.sampling_topp`): the shape of
tools/gen_ngram_bench.py (B videos x 5 events, beam 5, 60 tokens, min_len = max_len - 1 so that every arm runs the same
steps, device-side search, GPT-2-medium decoder or `DEC=txdec`) with four arms alternating in one process: beam search,
plain sampling, top-k 40 and top-p 0.9.  Each arm has its own search session; the decoder keeps only its two most
recent sessions, so the tool holds the four itself and hands the decoder the arm's own before every generation.
Timing starts at the third use of each session, when every step is a graph replay -- asserted per repetition.
Beside the generations, the launches of one scoring step alone at the same rows x vocabulary: `vs_beam_topk` (k = 2 * beam) and `vs_sample_token` in its three modes, timed by events over a loop.
Writes medians and spreads to profiles/gen_sampling.json (or `--out PATH`).  Informational, not bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vidsitu_amd import ops, synth_data
from vidsitu_amd.extended_config import get_cfg
from vidsitu_amd.mdl_selector import get_mdl_loss_eval

ap = argparse.ArgumentParser()
ap.add_argument("--videos", type=int, default=2)
ap.add_argument("--beam", type=int, default=5)
ap.add_argument("--max-len", type=int, default=60)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              "profiles", "gen_sampling.json"))
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
ARMS = {"beam": (False, -1, -1.0), "plain": (True, -1, -1.0), "topk40": (True, 40, -1.0), "topp0.9": (True, -1, 0.9)}


sessions = {arm: {} for arm in ARMS}  # the arm's search sessions, kept alive here


def decoders():
    return [m for m in mdl.modules() if "_vs_search_sessions" in m.__dict__]


def generate(arm):
    g = evl.cfg.gen
    g.sampling, g.sampling_topk, g.sampling_topp = ARMS[arm]
    for m in decoders():
        m.__dict__["_vs_search_sessions"] = dict(sessions[arm])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = evl.forward_one_batch(mdl, batch)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    (dec_mod,) = decoders()
    sessions[arm] = dict(dec_mod.__dict__["_vs_search_sessions"])
    (ses,) = sessions[arm].values()
    return dt, [tuple(v["tokens"]) for r in out for v in r["vb_output"].values()], ses


def summary(v):
    q = statistics.quantiles(v, n=4)
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "iqr": q[2] - q[0],
            "spread": max(v) - min(v), "samples": [round(x, 3) for x in v]}


for arm in ARMS:  # use 1 eager, use 2 captures the step graphs
    assert [generate(arm)[2].uses for _ in range(2)] == [1, 2]
ms = {arm: [] for arm in ARMS}
distinct = {}
for _ in range(args.reps):
    for arm in ARMS:
        dt, toks, ses = generate(arm)
        assert ses.uses >= 3 and len(ses.graphs) > 0 and (ses.strategy is None) == (arm == "beam"), (arm, ses.uses)
        ms[arm].append(dt)
        distinct[arm] = len(set(toks))

# ---- one scoring step alone: rows = videos * 5 events * beam, the tokenizer's vocabulary
rows, vocab = args.videos * 5 * args.beam, len(comm.gpt2_hf_tok)
tok = comm.gpt2_hf_tok
logits = torch.randn(rows, vocab, device=dev) * 4
cum = torch.randn(rows, device=dev)
state = torch.tensor([1, 0], dtype=torch.long, device=dev)
snap = ops.dropout_tick(state)
steps = {"vs_beam_topk": lambda: ops.beam_topk(logits, cum, None, 2 * args.beam, tok.pad(), tok.eos(), tok.unk())}
for arm, (_, topk, topp) in ARMS.items():
    if arm != "beam":
        steps[f"vs_sample_token {arm}"] = (lambda topk=topk, topp=topp: ops.sample_token(
            logits, cum, None, snap, tok.pad(), tok.eos(), tok.unk(), sampling_topk=topk, sampling_topp=topp))
step_us = {}
for name, fn in steps.items():
    for _ in range(5):
        fn()
    samples = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            fn()
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) * 1e3 / 50)
    step_us[name] = summary(samples)

base = step_us["vs_beam_topk"]["median"]
res = {"shape": {"videos": args.videos, "events": 5, "beam": args.beam, "max_len": args.max_len, "decoder": dec,
                 "device_search": True, "reps_per_arm": args.reps, "timed_from_use": 3, "rows": rows, "vocab": vocab},
       "generation_ms": {arm: summary(v) for arm, v in ms.items()},
       "generation_minus_beam_median_ms": {arm: statistics.median(v) - statistics.median(ms["beam"])
                                           for arm, v in ms.items() if arm != "beam"},
       "distinct_captions_of_10_events_x_beam_last_rep": distinct,
       # eager launches in a loop (workspace allocation included on both sides), events around 50 calls
       "scoring_step_us": step_us,
       "scoring_step_over_vs_beam_topk": {k: v["median"] / base for k, v in step_us.items()},
       "device": torch.cuda.get_device_name(0)}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
for arm, v in ms.items():
    s = summary(v)
    print(f"{arm}: median {s['median']:.2f} ms, min {s['min']:.2f}, max {s['max']:.2f}, iqr {s['iqr']:.2f}")
for k, v in step_us.items():
    print(f"{k}: median {v['median']:.1f} us ({v['median'] / base:.2f} x vs_beam_topk), spread {v['spread']:.1f}")
