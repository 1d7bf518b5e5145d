"""Host-side mirror of the reference's feature dump (`vidsitu_code/feat_extractor.py:76-112`,
SURVEY.md 8a row A8): trunk -> trimmed head -> one `[E, feat_dim]` float32 `.npy` per video, named
`<vseg_name>_feats.npy` under `<cfg.ds.vsitu.vsitu_frm_feats>/<mdl_name>/`, the format
`VsituDS.get_frm_feats_all` (`vidsitu_code/dat_loader.py:503-511`) reads back for the TxEncoder
models.  Same class / method names and the same loop; the model call runs on the HIP kernels.
"""
import queue
import threading
from pathlib import Path

import numpy as np
import torch

from . import synth_data
from ._lib import VsError


class SynthFrameDataset:
    """`VsituDS_All` stand-in (`feat_extractor.py:40-74`): `vseg_lst` names + `all_itemgetter`
    items of the A0 contract with seeded synthetic frames.  `frames`: "fp32" -- the reference's float tensors
    (N(0,1) noise, `synth_batch`); "u8" -- `frms_ev_fast_u8`, video-like uint8 frames at the crop size
    (`synth_video_u8_batch`); "raw_u8" -- `frms_ev_raw_u8`, the same at the source size `src_hw` = (H0, W0), as a
    decoder leaves them (the resize runs on the GPU)."""

    FRAME_MODES = ("fp32", "u8", "raw_u8")

    def __init__(self, cfg, comm, n_videos, n_ev=5, seed=0, crop=None, names=None, frames="fp32", src_hw=(256, 340)):
        if frames not in self.FRAME_MODES:
            raise ValueError(f"frames={frames!r}: one of {self.FRAME_MODES}")
        self.cfg, self.comm = cfg, comm
        self.n_ev, self.seed, self.crop = n_ev, seed, crop
        self.frames, self.src_hw = frames, (int(src_hw[0]), int(src_hw[1]))
        self.vseg_lst = names or [f"v_synth{ix:05d}_seg_0_10" for ix in range(n_videos)]

    def __len__(self):
        return len(self.vseg_lst)

    def __getitem__(self, idx):
        if self.frames == "fp32":
            b = synth_data.synth_batch(self.cfg, self.comm, bs=1, n_ev=self.n_ev, seed=self.seed + idx,
                                       crop=self.crop)
        else:
            raw = self.frames == "raw_u8"
            b = synth_data.synth_video_u8_batch(self.cfg, self.comm, bs=1, n_ev=self.n_ev, seed=self.seed + idx,
                                                crop=self.crop, hw=self.src_hw if raw else None)
            if raw:
                b["frms_ev_raw_u8"] = b.pop("frms_ev_fast_u8")
        out = {k: v[0] for k, v in b.items() if k.startswith("frms_")}
        out["vseg_idx"] = torch.tensor(idx).long()
        return out


class SimpleLoader:
    """Sequential batches with `.dataset` (the two attributes `forward_all` uses of a DataLoader);
    collate = stack per key (`utils/dat_utils.py:81-109` for tensors)."""

    def __init__(self, dataset, batch_size):
        self.dataset, self.batch_size = dataset, batch_size

    def __iter__(self):
        for i0 in range(0, len(self.dataset), self.batch_size):
            items = [self.dataset[i] for i in range(i0, min(len(self.dataset), i0 + self.batch_size))]
            yield {k: torch.stack([it[k] for it in items]) for k in items[0]}

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size


class FeatExtract:
    def __init__(self, cfg):
        self.cfg = cfg

    def set_mdl_dl(self, mdl, dl, mdl_name: str, split_name: str):
        self.mdl = mdl
        self.dl = dl
        self.mdl_name = mdl_name
        self.split_name = split_name
        out_tdir = Path(self.cfg.ds.vsitu.vsitu_frm_feats) / f"{mdl_name}"
        out_tdir.mkdir(exist_ok=True, parents=True)
        self.out_tdir = out_tdir

    @torch.no_grad()
    def forward_all(self, device=None, dtype=torch.bfloat16):
        """feat_extractor.py:90-112.  Frames go to the GPU as bf16 (the trunk's storage type)."""
        device = device or torch.device("cuda")
        vseg_lst = self.dl.dataset.vseg_lst
        written = []
        for batch in self.dl:
            batch_gpu = {k: (v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device))
                         for k, v in batch.items()}
            feat_out = self.mdl.forward_encoder(batch_gpu)
            head_out = self.mdl.head(feat_out)
            head_out = head_out.permute((0, 2, 3, 4, 1))  # (N, C, 1, 1, 1) -> (N, 1, 1, 1, C)
            B = len(batch["vseg_idx"])
            assert head_out.size(1) == 1 and head_out.size(2) == 1 and head_out.size(3) == 1
            n_ev = head_out.size(0) // B  # the reference's literal 5
            out_np = head_out.reshape(B, n_ev, -1).float().cpu().numpy()
            for vix in range(B):
                vseg_name = vseg_lst[int(batch["vseg_idx"][vix])]
                out_np_name = self.out_tdir / f"{vseg_name}_feats.npy"
                np.save(out_np_name, out_np[vix])
                written.append(out_np_name)
        return written

    def forward_all_stream(self, device=None, depth=2):
        """`forward_all` for loaders of uint8 frames (`frms_ev_raw_u8` / `frms_ev_fast_u8`), pipelined: same files, same
        bytes, same returned list.  See `_StreamRun`."""
        run = _StreamRun(self, device or torch.device("cuda"), int(depth))
        return run.run()


class _Slot:
    """One batch in flight: pinned host input, a captured forward with its static device input and output, pinned host
    output, and the events that order the three legs."""

    def __init__(self, mdl, batch, key, device, compute, direct):
        from .eval_graph import EvalGraph

        fr = batch[key]
        self.key = key
        self.host_in = None if direct else torch.empty(fr.shape, dtype=fr.dtype, pin_memory=True)
        self.src = None  # what the H2D reads: host_in, or the loader's own tensor when that is pinned already
        with torch.cuda.stream(compute):
            self.graph = EvalGraph.for_model(mdl, {key: fr.to(device)})
        self.host_out = torch.empty(self.graph.feats.shape, dtype=torch.float32, pin_memory=True)
        self.ev_in, self.ev_done, self.ev_out = (torch.cuda.Event() for _ in range(3))
        self.vseg = None


class _StreamRun:
    """One `forward_all_stream` call.  Three actors:

      producer thread  pulls batches from the loader and copies each into a free slot's pinned host buffer;
      caller's thread  H2D on the copy stream -> the compute stream waits for the copy's event and replays the slot's
                       `EvalGraph` -> D2H of the [B, E, C] features into pinned memory on the copy stream;
      writer thread    `np.save` per video, then frees the slot.

    One graph PER SLOT, so the H2D lands in the static input of the graph that will read it and the compute stream
    carries the forward alone.  Each graph keeps its own memory pool: in a shared one the output of one slot's graph
    may sit where another slot's graph keeps an intermediate, and that graph's next replay would overwrite features
    whose D2H is still queued.  `depth` slots
    exist per batch shape, made on first need (a short last batch gets one slot of its own).  Batches the loader has
    pinned already are copied to the device from where they are; pageable ones go through the slot's pinned buffer.  The caller's thread
    enqueues batch i+1 -- copy, wait, replay -- BEFORE it enqueues the D2H of batch i and waits for it: the only host
    wait is for the output of an earlier batch, and the H2D of batch i+1 runs while batch i computes.  That needs one
    slot more than batches in flight, so `depth=1` runs the three legs of each batch one after another.  The helper
    threads make no device call."""

    def __init__(self, fe, device, depth):
        if depth < 1:
            raise ValueError("depth must be at least 1")
        self.fe, self.device, self.depth = fe, device, depth
        self.inbox, self.to_write = queue.Queue(), queue.Queue()
        self.stop = threading.Event()
        self.pools = {}  # batch shape -> {"free": Queue of slots, "made": count}; created by the producer only
        self.slots = []
        self.written = []

    def _get(self, q):
        while not self.stop.is_set():
            try:
                return q.get(timeout=0.05)
            except queue.Empty:
                pass
        raise _Stopped()

    # ---- producer thread ----
    def _produce(self):
        try:
            for batch in self.fe.dl:
                keys = [k for k in ("frms_ev_raw_u8", "frms_ev_fast_u8") if k in batch]
                if len(keys) != 1 or batch[keys[0]].dtype != torch.uint8:
                    raise VsError("forward_all_stream takes batches of uint8 frames (`frms_ev_raw_u8` or "
                                  f"`frms_ev_fast_u8`), got {sorted(batch)}: use forward_all for the fp32 contract")
                fr = batch[keys[0]]
                shape = (keys[0],) + tuple(fr.shape)
                pool = self.pools.setdefault(shape, {"free": queue.Queue(), "made": 0})
                try:
                    slot = pool["free"].get_nowait()
                except queue.Empty:
                    if pool["made"] < self.depth:
                        pool["made"] += 1
                        self.inbox.put(("new_slot", pool, batch, keys[0]))
                    slot = self._get(pool["free"])
                if pool["direct"]:
                    slot.src = fr  # (kept alive by the slot until it is filled again)
                else:
                    slot.host_in.copy_(fr)
                    slot.src = slot.host_in
                slot.vseg, slot.pool = [int(v) for v in batch["vseg_idx"]], pool
                self.inbox.put(("filled", slot))
            self.inbox.put(("end",))
        except _Stopped:
            pass
        except BaseException as e:  # noqa: BLE001  (surfaces in the caller)
            self.inbox.put(("error", e))

    # ---- writer thread ----
    def _write(self):
        try:
            while True:
                slot = self._get(self.to_write)
                if slot is None:
                    return
                out_np = slot.host_out.numpy()
                for vix, name in enumerate(slot.names):
                    np.save(name, out_np[vix])
                slot.pool["free"].put(slot)
        except _Stopped:
            pass
        except BaseException as e:  # noqa: BLE001
            self.inbox.put(("error", e))

    # ---- caller's thread ----
    def _issue(self, slot):
        with torch.cuda.stream(self.copy):
            slot.graph.inp.copy_(slot.src, non_blocking=True)
            slot.ev_in.record(self.copy)
        self.compute.wait_event(slot.ev_in)
        with torch.cuda.stream(self.compute):
            slot.graph.replay()
            slot.ev_done.record(self.compute)
        vseg_lst = self.fe.dl.dataset.vseg_lst
        slot.names = [self.fe.out_tdir / f"{vseg_lst[v]}_feats.npy" for v in slot.vseg]
        self.written += slot.names

    def _finish(self, slot):
        self.copy.wait_event(slot.ev_done)
        with torch.cuda.stream(self.copy):
            slot.host_out.copy_(slot.graph.feats, non_blocking=True)
            slot.ev_out.record(self.copy)
        slot.ev_out.synchronize()
        self.to_write.put(slot)

    def run(self):
        self.copy, self.compute = torch.cuda.Stream(self.device), torch.cuda.Stream(self.device)
        self.compute.wait_stream(torch.cuda.current_stream(self.device))
        threads = [threading.Thread(target=self._produce, name="feat-stream-producer", daemon=True),
                   threading.Thread(target=self._write, name="feat-stream-writer", daemon=True)]
        for th in threads:
            th.start()
        prev, error = None, None
        try:
            while True:
                msg = self.inbox.get()
                if msg[0] == "error":
                    raise msg[1]
                if msg[0] == "new_slot":
                    _, pool, batch, key = msg
                    # a loader that pins its batches itself (DataLoader(pin_memory=True)) needs no staging copy; asked
                    # here, once per batch shape, because the helper threads make no device-runtime call
                    pool.setdefault("direct", batch[key].is_pinned())
                    slot = _Slot(self.fe.mdl, batch, key, self.device, self.compute, pool["direct"])
                    self.slots.append(slot)
                    pool["free"].put(slot)
                elif msg[0] == "filled":
                    self._issue(msg[1])
                    if prev is not None:
                        self._finish(prev)
                    prev = msg[1]
                    if self.depth == 1:  # one slot: nothing can be in flight beside it, and the producer waits for it
                        self._finish(prev)
                        prev = None
                else:  # "end"
                    if prev is not None:
                        self._finish(prev)
                    break
            self.to_write.put(None)
            threads[1].join()
            while not self.inbox.empty():  # a failure of the writer's last saves
                msg = self.inbox.get()
                if msg[0] == "error":
                    raise msg[1]
        except BaseException as e:  # noqa: BLE001
            error = e
        finally:
            self.stop.set()
            for th in threads:
                th.join()
            self.copy.synchronize()
            self.compute.synchronize()
            torch.cuda.current_stream(self.device).wait_stream(self.compute)
            # release the graphs HERE, with nothing in flight: slot <-> pool is a reference cycle, and a graph the
            # cycle collector destroys later, during somebody's capture, invalidates that capture
            for slot in self.slots:
                slot.graph = slot.pool = slot.src = None
            self.slots.clear()
            self.pools.clear()
        if error is not None:
            raise error
        return self.written


class _Stopped(Exception):
    pass


def read_frm_feats(feats_dir, vseg_name):
    """`VsituDS.get_frm_feats_all` (`dat_loader.py:503-511`): -> {"frm_feats": f32 [E, D]}."""
    arr = np.load(Path(feats_dir) / f"{vseg_name}_feats.npy")
    return {"frm_feats": torch.from_numpy(arr).float()}


def main(mdl_resume_path: str, mdl_name_used: str, is_cu: bool = False, splits=("valid", "train"), n_videos=None,
         calibrate: int = 2, frames: str = "fp32", src_hw=(256, 340), stream: int = 0, **kwargs):
    """`python -m vidsitu_amd.feat_extractor <weights> <name> [--is_cu=True] [--dotted.key=value ...]`
    (`feat_extractor.py:119-176`): build the configured model, load a TRAINED checkpoint (the trainer's file format,
    `module.` prefixes stripped) or -- `is_cu` -- the Kinetics model-zoo Caffe2 pickle into `mdl.sf_mdl`, and write
    `<vsitu_frm_feats>/<name>/<vseg>_feats.npy` ([E, 2304] / [E, 2048] float32) for every video of every split.
    The videos are the synthetic stand-in dataset (`SynthFrameDataset`; the 50 GB frame dataset is out of scope), so what this
    entry point pins is the flow: weights -> eval trunk on the HIP kernels -> head -> files the TxEncoder rows read back.
    `--calibrate=N` (default 2; 0 = off, the reference's behaviour: it has no such step): before the first split the
    model measures, on the clips of the first N videos OF THE DATASET BEING EXTRACTED (the first split's loader -- the
    evaluation distribution itself, never a stand-in: a constant measured on other data is a data-dependent bias, not a
    correction), the per-channel constants the bf16 rounding of its convolution weights adds and folds their correction
    into the BN shifts (`SFBase.calibrate_weight_rounding`): features within 1e-3 of the fp32 reference's instead of
    3e-3 (tests/test_gpu_parity_full.py; spread over clips and under a calibration / evaluation distribution shift:
    profiles/parity_eval.json), at no cost per forward.  Calibration must precede any hipGraph capture of the eval
    forward: a captured graph keeps the fold tensors it was recorded with (`eval_graph.EvalGraph` refuses to replay
    one captured before).
    `--frames=fp32|u8|raw_u8` (default fp32, the reference's contract): what the stand-in dataset yields -- float tensors,
    uint8 frames at the crop size, or uint8 frames at `--src_hw=HxW` (default 256x340) that the GPU resizes.
    `--stream=1` (uint8 frames only): `FeatExtract.forward_all_stream`, the pipelined extractor; the files are the
    same."""
    if int(stream) and frames == "fp32":
        raise ValueError("--stream=1 takes uint8 frames: pass --frames=u8 or --frames=raw_u8")
    from . import checkpoint, synth_data
    from .extended_config import get_cfg
    from .mdl_selector import get_mdl_loss_eval

    cfg = get_cfg(kwargs)
    cfg.num_gpus, cfg.do_dist = 1, False
    comm = synth_data.make_comm(cfg)
    mdl = get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=comm)
    if is_cu:
        print("Using Caffe2 checkpoint")
        cfg.sf_mdl.TRAIN.CHECKPOINT_FILE_PATH, cfg.sf_mdl.TRAIN.CHECKPOINT_TYPE = mdl_resume_path, "caffe2"
        checkpoint.load_sf_pretrained(cfg, mdl)
    else:
        got = checkpoint.load_model_dict(mdl_resume_path, mdl, None, load_opt=False, strict=True)
        if got is None:
            raise FileNotFoundError(mdl_resume_path)
    mdl = mdl.to(torch.device("cuda")).eval()
    feat_ext, written = FeatExtract(cfg), []
    n = int(n_videos) if n_videos is not None else int(cfg.synth.num_videos)
    for si, split in enumerate(splits):
        ds = SynthFrameDataset(cfg, comm, n, n_ev=cfg.ds.vsitu.num_ev, seed=cfg.synth.seed + 1000 * si,
                               names=[f"{split}_v{i:05d}_seg_0-10" for i in range(n)], frames=frames, src_hw=src_hw)
        if si == 0 and int(calibrate) > 0 and hasattr(mdl, "calibrate_weight_rounding"):
            n_vid = min(int(calibrate), len(ds))
            cal = next(iter(SimpleLoader(ds, n_vid)))
            cal = {k: (v.to(device="cuda", dtype=torch.bfloat16) if v.is_floating_point() else v.to("cuda"))
                   for k, v in cal.items()}
            n_cal = mdl.calibrate_weight_rounding(cal)
            print(f"weight-rounding correction calibrated on the first {n_vid} video(s) of split {split!r}: "
                  f"{n_cal} convolutions")
        feat_ext.set_mdl_dl(mdl, SimpleLoader(ds, max(1, int(cfg.train.bsv))), mdl_name=mdl_name_used, split_name=split)
        written += feat_ext.forward_all_stream() if int(stream) else feat_ext.forward_all()
    print(f"wrote {len(written)} feature files under {feat_ext.out_tdir}")
    return written


USAGE = ("usage: python -m vidsitu_amd.feat_extractor <weights> <name> [--is_cu=True] [--frames=fp32|u8|raw_u8] "
         "[--src_hw=HxW] [--stream=0|1] [--dotted.key=value ...]")


def parse_args(argv):
    """`argv` without the program name -> (weights path, model name, keyword arguments of `main`)."""
    if len(argv) < 2:
        raise SystemExit(USAGE)
    kw = {}
    for a in argv[2:]:
        if not a.startswith("--") or "=" not in a:
            raise SystemExit(f"{a!r}: options are --key=value\n{USAGE}")
        k, v = a[2:].split("=", 1)
        kw[k] = v
    kw["is_cu"] = str(kw.pop("is_cu", "False")) in ("1", "True", "true")
    if "calibrate" in kw:
        kw["calibrate"] = int(kw["calibrate"])
    if "splits" in kw:
        kw["splits"] = tuple(kw["splits"].split(","))
    if "frames" in kw and kw["frames"] not in SynthFrameDataset.FRAME_MODES:
        raise SystemExit(f"--frames={kw['frames']}: one of {', '.join(SynthFrameDataset.FRAME_MODES)}")
    if "src_hw" in kw:
        try:
            h, w = (int(x) for x in kw["src_hw"].lower().split("x"))
            assert h > 0 and w > 0
        except (ValueError, AssertionError):
            raise SystemExit(f"--src_hw={kw['src_hw']}: HEIGHTxWIDTH, e.g. 256x340") from None
        kw["src_hw"] = (h, w)
    if "stream" in kw:
        if kw["stream"] not in ("0", "1"):
            raise SystemExit(f"--stream={kw['stream']}: 0 or 1")
        kw["stream"] = int(kw["stream"])
        if kw["stream"] and kw.get("frames", "fp32") == "fp32":
            raise SystemExit("--stream=1 takes uint8 frames: add --frames=u8 or --frames=raw_u8")
    return argv[0], argv[1], kw


if __name__ == "__main__":
    import sys

    weights, name, kw = parse_args(sys.argv[1:])
    main(weights, name, **kw)
