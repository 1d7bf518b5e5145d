"""What a diverse beam search costs a generation (`gen.diverse_beam_groups`, `gen.diversity_rate`): the shape of
tools/gen_sampling_bench.py (B videos x 5 events, beam 5, 60 tokens, min_len = max_len - 1 so that every arm runs the
same steps, device-side search, GPT-2-medium decoder or `DEC=txdec`) with three arms alternating in one process: beam
search, groups (G = beam, strength 0.5) and siblings (rate 0.5).  Each arm has its own search session; the decoder
keeps only its two most recent sessions, so the tool holds the three itself and hands the decoder the arm's own before
every generation.  Timing starts at the third use of each session, when every step is a graph replay -- asserted per
repetition.  Beside the generations, the bookkeeping kernels of one step alone at videos x 5 x beam rows:
`vs_beam_step` and `vs_beam_diverse_step` in both modes on the same lists, timed by events over a loop.
`--arms beam` runs the beam-search leg alone (this is how the tool runs on a checkout from before the feature);
`--parent PATH` copies that run's beam-search summary into the output beside this run's.
Writes medians and spreads to profiles/gen_diverse.json (or `--out PATH`).  Informational, not bench.py."""
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
ap.add_argument("--arms", default="beam,groups,siblings")
ap.add_argument("--parent", default=None, help="JSON of a `--arms beam` run on the parent checkout")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              "profiles", "gen_diverse.json"))
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
# (diverse_beam_groups, diverse_beam_strength, diversity_rate) and the session's strategy key
ALL = {"beam": ((-1, 0.5, -1.0), None), "groups": ((args.beam, 0.5, -1.0), ("groups", args.beam, 0.5)),
       "siblings": ((-1, 0.5, 0.5), ("siblings", 0.5))}
ARMS = {arm: ALL[arm] for arm in args.arms.split(",")}

sessions = {arm: {} for arm in ARMS}  # the arm's search sessions, kept alive here


def decoders():
    return [m for m in mdl.modules() if "_vs_search_sessions" in m.__dict__]


def generate(arm):
    g = evl.cfg.gen
    if arm != "beam" or "diverse_beam_groups" in g:  # a checkout from before the feature has no such keys
        g.diverse_beam_groups, g.diverse_beam_strength, g.diversity_rate = ARMS[arm][0]
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
captions = {}
for _ in range(args.reps):
    for arm in ARMS:
        dt, toks, ses = generate(arm)
        assert ses.uses >= 3 and len(ses.graphs) > 0 and ses.strategy == ARMS[arm][1], (arm, ses.uses, ses.strategy)
        ms[arm].append(dt)
        captions[arm] = toks

# ---- the bookkeeping kernel of one step alone: rows = videos * 5 events * beam, lists of 2 * beam entries
bsz, beam, vocab = args.videos * 5, args.beam, len(comm.gpt2_hf_tok)
rows, k, max_len, step = bsz * beam, 2 * args.beam, args.max_len, args.max_len // 2
tok = comm.gpt2_hf_tok
gen = torch.Generator(device="cpu").manual_seed(0)
row_val = torch.sort(torch.randn(rows, k, generator=gen) * 2 - 40, dim=1, descending=True)[0].to(dev)
live = torch.tensor([t for t in range(vocab) if t not in (tok.pad(), tok.eos())])  # no eos: no sentence finishes
row_idx = torch.stack([live[torch.randperm(live.numel(), generator=gen)[:k]] for _ in range(rows)]).to(dev)
i64, f32, i32, u8 = torch.long, torch.float32, torch.int32, torch.uint8
buf = dict(tok=[torch.full((rows, max_len + 2), 7, dtype=i64, device=dev) for _ in range(2)],
           sc=[torch.zeros((rows, max_len + 1), dtype=f32, device=dev) for _ in range(2)],
           anc=[torch.arange(rows, dtype=i32, device=dev).view(-1, 1).repeat(1, max_len + 2) for _ in range(2)],
           ignore=torch.zeros((bsz, beam), dtype=u8, device=dev), finished=torch.zeros(bsz, dtype=u8, device=dev),
           nfin=torch.zeros(bsz, dtype=i32, device=dev), remaining=torch.full((1,), bsz, dtype=i32, device=dev),
           fin_tok=torch.zeros((bsz, beam, max_len + 1), dtype=i64, device=dev),
           fin_score=torch.zeros((bsz, beam), dtype=f32, device=dev),
           fin_pos=torch.zeros((bsz, beam, max_len + 1), dtype=f32, device=dev),
           fin_len=torch.zeros((bsz, beam), dtype=i32, device=dev), reorder=torch.zeros(rows, dtype=i64, device=dev))


def launch(fn, *tail):
    b = buf
    fn(row_val, row_idx, b["tok"][0], b["tok"][1], b["sc"][0], b["sc"][1], b["ignore"], b["finished"], b["nfin"],
       b["remaining"], b["fin_tok"], b["fin_score"], b["fin_pos"], b["fin_len"], b["reorder"], bsz, beam, k, vocab,
       step, max_len, tok.eos(), True, 1.0, *tail, anc_in=b["anc"][0], anc_out=b["anc"][1])


steps = {"vs_beam_step": lambda: launch(ops.beam_step)}
if hasattr(ops, "beam_diverse_step"):
    steps["vs_beam_diverse_step groups=1 strength=0"] = lambda: launch(ops.beam_diverse_step, 1, 0.0, 0.0)
    steps[f"vs_beam_diverse_step groups={beam} strength=0.5"] = lambda: launch(ops.beam_diverse_step, beam, 0.5, 0.0)
    steps["vs_beam_diverse_step siblings rate=0.5"] = lambda: launch(ops.beam_diverse_step, 0, 0.0, 0.5)
step_us = {}
for name, fn in steps.items():
    for _ in range(5):
        fn()
    samples = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            fn()
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) * 1e3 / 200)
    step_us[name] = summary(samples)
assert int(buf["remaining"]) == bsz  # no list holds eos: no sentence finished, every launch did the whole step

base = step_us["vs_beam_step"]["median"]
res = {"shape": {"videos": args.videos, "events": 5, "beam": args.beam, "max_len": args.max_len, "decoder": dec,
                 "device_search": True, "reps_per_arm": args.reps, "timed_from_use": 3, "rows": rows, "vocab": vocab},
       "generation_ms": {arm: summary(v) for arm, v in ms.items()},
       "generation_minus_beam_median_ms": {arm: statistics.median(v) - statistics.median(ms["beam"])
                                           for arm, v in ms.items() if arm != "beam" and "beam" in ms},
       # of videos * 5 events, one caption each (the best hypothesis): how many differ from the beam search's
       "captions_differing_from_beam_last_rep": {arm: sum(a != b for a, b in zip(captions[arm], captions["beam"]))
                                                 for arm in captions if arm != "beam" and "beam" in captions},
       # launches in a loop (a launch-bound kernel: this is the time between launches), events around 200 calls
       "bookkeeping_step_us": step_us,
       "bookkeeping_step_minus_vs_beam_step_us": {name: v["median"] - base for name, v in step_us.items()},
       "device": torch.cuda.get_device_name(0)}
if args.parent:
    with open(args.parent) as f:
        parent = json.load(f)
    res["parent_checkout"] = {"generation_ms": {"beam": parent["generation_ms"]["beam"]},
                              "bookkeeping_step_us": parent["bookkeeping_step_us"]}
    res["beam_median_minus_parent_ms"] = (res["generation_ms"]["beam"]["median"]
                                          - parent["generation_ms"]["beam"]["median"])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
for arm, v in ms.items():
    s = summary(v)
    print(f"{arm}: median {s['median']:.2f} ms, min {s['min']:.2f}, max {s['max']:.2f}, iqr {s['iqr']:.2f}")
for name, v in step_us.items():
    print(f"{name}: median {v['median']:.1f} us ({v['median'] - base:+.1f} vs vs_beam_step), spread {v['spread']:.1f}")
