"""End-to-end feature extraction from host-resident frames, one GPU visit, one JSON line (profiles/feat_stream.json).

SlowFast-R50, eval, 8 clips per batch (2 videos x 4 events), frames pre-generated and resident in host memory so
that the dataset's own cost is out of the picture.  clips/s of
  (a) `forward_all` as it always was: fp32 pageable batches, blocking `.to()`, eager model, `.cpu()` + `np.save` in line;
  (b) `forward_all_stream` on 224^2 uint8 frames (`frms_ev_fast_u8`);
  (c) `forward_all_stream` on 256x340 decoded frames (`frms_ev_raw_u8`, fused ingest);
  (d) the captured forward of (b) and of (c) replayed on device-resident input: the ceilings;
the H2D rate (b) and (c) achieve and the rate of a plain pinned copy of the same size in this process; and the fused
ingest launch against the four-launch chain it replaces (resize h, resize v, pack per pathway), each captured in a
hipGraph and replayed ALTERNATELY, median of `--replays` replays, at three source sizes.

    python tools/feat_stream_bench.py [--batches 24] [--replays 30] [--out profiles/feat_stream.json]
"""
import argparse
import gc
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vidsitu_amd import ops, synth_data  # noqa: E402
from vidsitu_amd.eval_graph import EvalGraph  # noqa: E402
from vidsitu_amd.extended_config import get_cfg  # noqa: E402
from vidsitu_amd.feat_extractor import FeatExtract  # noqa: E402
from vidsitu_amd.mdl_selector import get_mdl_loss_eval  # noqa: E402

B, E = 2, 4


class _Names:
    def __init__(self, n):
        self.vseg_lst = [f"bench_v{i:05d}" for i in range(n)]


class ResidentLoader:
    """`n_batches` batches cycling over a few pre-generated host-resident ones."""

    def __init__(self, protos, n_batches):
        self.protos, self.n = protos, n_batches
        self.dataset = _Names(n_batches * B)

    def __len__(self):
        return self.n

    def __iter__(self):
        for i in range(self.n):
            b = dict(self.protos[i % len(self.protos)])
            b["vseg_idx"] = torch.arange(i * B, (i + 1) * B)
            yield b


def u8_protos(cfg, comm, hw, key, k=2):
    out = []
    for s in range(k):
        fr = synth_data.synth_video_u8_batch(cfg, comm, bs=B, n_ev=E, seed=50 + s, hw=hw)["frms_ev_fast_u8"]
        out.append({key: fr.pin_memory()})
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 3), "min": round(v[0], 3), "max": round(v[-1], 3),
            "p25": round(v[len(v) // 4], 3), "p75": round(v[(3 * len(v)) // 4], 3)}


def copy_bandwidth(nbytes, dev, reps=10):
    h = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    d = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d.copy_(h, non_blocking=True)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        d.copy_(h, non_blocking=True)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return nbytes / (statistics.median(ts) * 1e-3) / 1e9


def ingest_vs_chain(dev, h0, w0, frames, replays, mean, std):
    t = 32
    n = max(1, frames // t)
    gc.collect()  # (no graph of an earlier stage may be destroyed by the collector during the captures below)
    fr = torch.randint(0, 256, (n, t, h0, w0, 3), dtype=torch.uint8, device=dev)
    tidx = torch.linspace(0, t - 1, t // 4).long().to(torch.int32).to(dev)

    def fused():
        return ops.ingest_u8(fr, 224, 224, 4, tidx, 4, mean, std)

    def chain():
        r = ops.resize_bicubic_u8(fr, 224, 224)
        return ops.frames_u8_pack(r, 4, None, mean, std), ops.frames_u8_pack(r, 4, tidx, mean, std)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graphs, outs = {}, {}
    with torch.cuda.stream(side):
        for name, fn in (("fused", fused), ("chain", chain)):
            for _ in range(3):
                fn()
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                outs[name] = fn()
            graphs[name] = g
        for g in graphs.values():
            g.replay()
        side.synchronize()
        same = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(outs["fused"], outs["chain"]))
        ts = {"fused": [], "chain": []}
        for _ in range(replays):
            for name in ("chain", "fused"):  # alternating
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(side)
                graphs[name].replay()
                b.record(side)
                b.synchronize()
                ts[name].append(a.elapsed_time(b) * 1e3)
    src_mb = fr.numel() / 1e6
    out_mb = sum(o.numel() * 2 for o in outs["fused"]) / 1e6
    f, c = spread(ts["fused"]), spread(ts["chain"])
    return {"src_hw": [h0, w0], "frames": n * t, "bitwise_equal": bool(same), "fused_us": f, "chain_us": c,
            "fused_over_chain": round(f["median"] / c["median"], 3),
            "fused_needed_MB": round(src_mb + out_mb, 1),
            "fused_TBps_of_needed_bytes": round((src_mb + out_mb) / f["median"], 2)}  # MB / us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="recorded in the output when the tree has no history of its own")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("feat_stream_bench needs a GPU (nothing here is measured without one)")
    dev = torch.device("cuda:0")
    cfg = get_cfg({"mdl.mdl_name": "sf_base"})
    comm = synth_data.make_comm(cfg)
    torch.manual_seed(0)
    mdl = get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=comm).to(dev).eval()
    tmp = tempfile.mkdtemp(prefix="feat_stream_bench_")
    cfg.ds.vsitu.vsitu_frm_feats = tmp
    fe = FeatExtract(cfg)
    nb = args.batches
    res = {"tool": "tools/feat_stream_bench.py", "model": "SlowFast-R50 (sf_base), eval, random init",
           "clips_per_batch": B * E, "batches": nb, "device": torch.cuda.get_device_name(0)}
    try:
        res["commit"] = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL,
                                                cwd=os.path.dirname(os.path.abspath(__file__))).decode().strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        res["commit"] = None
    res["commit"] = args.commit or res["commit"]
    res["notes"] = ("steady_* = (time of a 2N-batch call - median time of an N-batch call) / N, three of each, alternating: "
                    "a call's fixed cost (warm-up and capture of its slots' graphs) is in whole_call_* only. "
                    "bound_clips_per_s = min(d of the same input kind, pinned copy rate / bytes per clip). *_staged: "
                    "pageable batches, one host memcpy per batch into the slot's pinned buffer on the producer thread. "
                    "ingest_fused_vs_chain: microseconds per graph replay, chain = resize h + resize v + pack x 2, "
                    "replays alternate.")

    # (a) fp32 pageable, forward_all
    fp = [{k: v for k, v in synth_data.synth_batch(cfg, comm, bs=B, n_ev=E, seed=70 + s).items()
           if k.startswith("frms_")} for s in range(2)]
    fe.set_mdl_dl(mdl, ResidentLoader(fp, 3), "a_warm", "bench")
    fe.forward_all(device=dev)
    na = max(4, nb // 3)
    runs = []
    for _ in range(3):
        fe.set_mdl_dl(mdl, ResidentLoader(fp, na), "a", "bench")
        runs.append(timed(lambda: fe.forward_all(device=dev)) / na)
    res["a_forward_all_fp32_pageable"] = {"clips_per_s": round(B * E / statistics.median(runs), 1),
                                          "ms_per_batch": spread([r * 1e3 for r in runs]), "batches": na}
    del fp

    def stream_leg(protos, key, tag):
        """Three N-batch calls and three 2N-batch calls, alternating; steady = (a 2N call - the median N call) / N."""
        nbytes = protos[0][key].numel()
        short, long_ = [], []
        for _ in range(3):
            fe.set_mdl_dl(mdl, ResidentLoader(protos, nb), tag, "bench")
            short.append(timed(lambda: fe.forward_all_stream(device=dev)))
            fe.set_mdl_dl(mdl, ResidentLoader(protos, 2 * nb), tag, "bench")
            long_.append(timed(lambda: fe.forward_all_stream(device=dev)))
        dt1 = statistics.median(short)
        per = [(d2 - dt1) / nb for d2 in long_]
        med = statistics.median(per)
        return {"bytes_per_batch": nbytes, "whole_call_s": [round(r, 4) for r in short],
                "whole_call_clips_per_s": round(nb * B * E / dt1, 1),
                "steady_ms_per_batch": spread([p * 1e3 for p in per]),
                "steady_clips_per_s": round(B * E / med, 1), "steady_h2d_GBps": round(nbytes / med / 1e9, 2)}

    def graph_leg(protos, key):
        """(d): the same captured forward replayed on device-resident input."""
        gc.collect()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            g = EvalGraph.for_model(mdl, {key: protos[0][key].to(dev)})
            g.replay()
            side.synchronize()
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(nb):
                    g.replay()
                side.synchronize()
                ts.append((time.perf_counter() - t0) / nb)
        del g
        return {"ms_per_batch": spread([t * 1e3 for t in ts]), "clips_per_s": round(B * E / statistics.median(ts), 1)}

    # (b), (c): batches the loader pinned (copied to the device from where they are); "_staged": the same batches
    # pageable, so the producer thread copies each into the slot's pinned buffer first; (d) per input kind
    for tag, hw, key in (("b_stream_u8_224", (224, 224), "frms_ev_fast_u8"),
                         ("c_stream_raw_u8_256x340", (256, 340), "frms_ev_raw_u8")):
        protos = u8_protos(cfg, comm, hw, key)
        bw = copy_bandwidth(protos[0][key].numel(), dev)
        d = graph_leg(protos, key)
        res["d_graph_replay_device_resident_" + key] = d
        pageable = [{key: p[key].clone()} for p in protos]
        for name, pr in ((tag, protos), (tag + "_staged", pageable)):
            r = stream_leg(pr, key, name)
            r["pinned_copy_GBps_same_size"] = round(bw, 2)
            bound = min(d["clips_per_s"], bw * 1e9 / (r["bytes_per_batch"] / (B * E)))
            r["bound_clips_per_s"] = round(bound, 1)
            r["steady_over_bound"] = round(r["steady_clips_per_s"] / bound, 3)
            res[name] = r
        del protos, pageable

    mean, std = tuple(cfg.sf_mdl.DATA.MEAN), tuple(cfg.sf_mdl.DATA.STD)
    res["ingest_fused_vs_chain"] = [ingest_vs_chain(dev, h0, w0, 256, args.replays, mean, std)
                                    for h0, w0 in ((256, 340), (360, 640), (1080, 1920))]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
