"""Streaming feature extraction (`FeatExtract.forward_all_stream`) against `forward_all` on the fp32 batch built from
the same frames on the host (resize oracle + `reference_tensors`): same files, same bytes, same list; and the
version check of `EvalGraph` around `calibrate_weight_rounding`."""
import numpy as np
import pytest
import torch

from oracle import resize_ref

pytestmark = pytest.mark.gpu

N_VIDEOS, N_EV, BATCH = 7, 2, 2  # 4 batches, the last one short


def _setup(name, dev, tmp_path, tag):
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    cfg = get_cfg({"mdl.sf_mdl_name": name, "synth.num_verbs": 23})
    cfg.ds.vsitu.vsitu_frm_feats = str(tmp_path / tag)
    comm = synth_data.make_comm(cfg)
    torch.manual_seed(0)
    mdl = get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=comm).to(dev).eval()
    return cfg, comm, mdl


class _Fp32Of:
    """The fp32 dataset of the reference's contract built from a uint8 dataset's frames on the host."""

    def __init__(self, ds, cfg, comm, crop):
        self.ds, self.cfg, self.comm, self.crop, self.vseg_lst = ds, cfg, comm, crop, ds.vseg_lst

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        from vidsitu_amd import synth_data

        it = self.ds[i]
        if "frms_ev_raw_u8" in it:
            raw = it["frms_ev_raw_u8"].numpy()
            fr = np.stack([resize_ref.resize_bicubic_u8(f, self.crop, self.crop)
                           for f in raw.reshape((-1,) + raw.shape[-3:])])
            fr = torch.from_numpy(fr).view(raw.shape[:2] + (self.crop, self.crop, 3))
        else:
            fr = it["frms_ev_fast_u8"]
        ref = synth_data.reference_tensors({"frms_ev_fast_u8": fr[None], "vseg_idx": it["vseg_idx"][None],
                                            "label_tensor": torch.zeros(1, fr.shape[0], dtype=torch.long)},
                                           self.cfg, self.comm)
        out = {k: v[0] for k, v in ref.items() if k.startswith("frms_")}
        out["vseg_idx"] = it["vseg_idx"]
        return out


@pytest.mark.parametrize("frames", ["raw_u8", "u8"])
@pytest.mark.parametrize("name", ["slow_fast_mini", "i3d_tiny"])
def test_stream_writes_the_files_of_forward_all(name, frames, dev, tmp_path):
    from vidsitu_amd.feat_extractor import FeatExtract, SimpleLoader, SynthFrameDataset

    cfg, comm, mdl = _setup(name, dev, tmp_path, "feats")
    crop = int(cfg.sf_mdl.DATA.TRAIN_CROP_SIZE)
    ds = SynthFrameDataset(cfg, comm, N_VIDEOS, n_ev=N_EV, seed=11, crop=crop, frames=frames, src_hw=(45, 80))
    fe = FeatExtract(cfg)
    fe.set_mdl_dl(mdl, SimpleLoader(_Fp32Of(ds, cfg, comm, crop), BATCH), mdl_name="ref", split_name="valid")
    want_paths = fe.forward_all(device=dev)
    want = [np.load(p) for p in want_paths]
    assert len(want) == N_VIDEOS and want[0].dtype == np.float32 and want[0].shape[0] == N_EV

    fe.set_mdl_dl(mdl, SimpleLoader(ds, BATCH), mdl_name="stream", split_name="valid")
    got_paths = fe.forward_all_stream(device=dev)
    assert [p.name for p in got_paths] == [p.name for p in want_paths]
    assert [p.parent for p in got_paths] == [fe.out_tdir] * N_VIDEOS
    first = [p.read_bytes() for p in got_paths]
    for p, w in zip(got_paths, want):
        g = np.load(p)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), p.name

    for depth in (3, 1):  # again: identical bytes, whatever the depth (1 = no overlap, one slot)
        again = fe.forward_all_stream(device=dev, depth=depth)
        assert again == got_paths
        assert [p.read_bytes() for p in again] == first


class _PinnedLoader:
    """A loader that pins its batches itself (`DataLoader(pin_memory=True)`): the extractor copies from them directly."""

    def __init__(self, inner):
        self.inner, self.dataset = inner, inner.dataset

    def __len__(self):
        return len(self.inner)

    def __iter__(self):
        for b in self.inner:
            yield {k: v.pin_memory() for k, v in b.items()}


@pytest.mark.parametrize("depth", [1, 2])
def test_stream_from_a_pinned_loader_writes_the_same_files(depth, dev, tmp_path):
    from vidsitu_amd.feat_extractor import FeatExtract, SimpleLoader, SynthFrameDataset

    cfg, comm, mdl = _setup("slow_fast_mini", dev, tmp_path, "feats")
    crop = int(cfg.sf_mdl.DATA.TRAIN_CROP_SIZE)
    ds = SynthFrameDataset(cfg, comm, N_VIDEOS, n_ev=N_EV, seed=5, crop=crop, frames="raw_u8", src_hw=(45, 80))
    fe = FeatExtract(cfg)
    fe.set_mdl_dl(mdl, SimpleLoader(ds, BATCH), mdl_name="staged", split_name="valid")
    want = [p.read_bytes() for p in fe.forward_all_stream(device=dev)]
    fe.set_mdl_dl(mdl, _PinnedLoader(SimpleLoader(ds, BATCH)), mdl_name="pinned", split_name="valid")
    got = fe.forward_all_stream(device=dev, depth=depth)
    assert len(got) == N_VIDEOS and [p.read_bytes() for p in got] == want


def test_eval_graph_refuses_to_replay_after_a_train_mode_pass(dev, tmp_path):
    """A train-mode pass rewrites the running statistics but folds nothing: the folds go stale BEFORE any re-fold runs."""
    from vidsitu_amd import _lib, synth_data
    from vidsitu_amd.eval_graph import EvalGraph

    cfg, comm, mdl = _setup("slow_fast_mini", dev, tmp_path, "feats")
    fr = synth_data.synth_video_u8_batch(cfg, comm, bs=1, n_ev=2, seed=1, hw=(45, 80))["frms_ev_fast_u8"].to(dev)
    batch = {"frms_ev_raw_u8": fr}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = EvalGraph.for_model(mdl, batch)
        g.replay()
    side.synchronize()
    mdl.train()
    with torch.no_grad():
        mdl.forward_encoder(batch)
    mdl.eval()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with pytest.raises(_lib.VsError, match="stale eval graph"):
            g.replay()
        with torch.no_grad():
            mdl.forward_encoder(batch)  # the eager forward re-folds; the old graph stays refused
        with pytest.raises(_lib.VsError, match="stale eval graph"):
            g.replay()
        g2 = EvalGraph.for_model(mdl, batch)
        g2.replay()
        got = g2.feats.clone()
    side.synchronize()
    with torch.no_grad():
        want = mdl.head(mdl.forward_encoder(batch)).view(1, 2, -1)
    assert torch.equal(got, want)
    # a parameter update (an optimizer step, a state_dict load) is seen the same way
    with torch.no_grad():
        next(mdl.sf_mdl.parameters()).mul_(1.0)
    with torch.cuda.stream(side):
        with pytest.raises(_lib.VsError, match="stale eval graph"):
            g2.replay()
    side.synchronize()


def test_stream_refuses_an_fp32_loader(dev, tmp_path):
    from vidsitu_amd import _lib
    from vidsitu_amd.feat_extractor import FeatExtract, SimpleLoader, SynthFrameDataset

    cfg, comm, mdl = _setup("slow_fast_mini", dev, tmp_path, "feats")
    ds = SynthFrameDataset(cfg, comm, 2, n_ev=N_EV, crop=int(cfg.sf_mdl.DATA.TRAIN_CROP_SIZE))
    fe = FeatExtract(cfg)
    fe.set_mdl_dl(mdl, SimpleLoader(ds, BATCH), mdl_name="fp32", split_name="valid")
    with pytest.raises(_lib.VsError, match="forward_all"):
        fe.forward_all_stream(device=dev)


def test_stream_surfaces_a_loader_failure(dev, tmp_path):
    from vidsitu_amd.feat_extractor import FeatExtract, SimpleLoader, SynthFrameDataset

    cfg, comm, mdl = _setup("i3d_tiny", dev, tmp_path, "feats")
    ds = SynthFrameDataset(cfg, comm, 5, n_ev=N_EV, crop=int(cfg.sf_mdl.DATA.TRAIN_CROP_SIZE), frames="u8")

    class Broken(SimpleLoader):
        def __iter__(self):
            for i, b in enumerate(super().__iter__()):
                if i == 2:
                    raise OSError("frame file went away")
                yield b

    fe = FeatExtract(cfg)
    fe.set_mdl_dl(mdl, Broken(ds, 1), mdl_name="broken", split_name="valid")
    with pytest.raises(OSError, match="went away"):
        fe.forward_all_stream(device=dev)
    import threading

    assert not [t for t in threading.enumerate() if t.name.startswith("feat-stream")]


@pytest.mark.parametrize("name", ["slow_fast_mini", "i3d_tiny"])
def test_eval_graph_and_calibration(name, dev, tmp_path):
    from vidsitu_amd import _lib, synth_data
    from vidsitu_amd.eval_graph import EvalGraph

    cfg, comm, mdl = _setup(name, dev, tmp_path, "feats")
    crop = int(cfg.sf_mdl.DATA.TRAIN_CROP_SIZE)
    mk = lambda seed: synth_data.synth_video_u8_batch(cfg, comm, bs=1, n_ev=2, seed=seed, hw=(45, 80))["frms_ev_fast_u8"]
    batch = {"frms_ev_raw_u8": mk(1).to(dev)}
    other = {"frms_ev_raw_u8": mk(2).to(dev)}
    cal = {"frms_ev_raw_u8": mk(3).to(dev)}

    def eager(b):
        with torch.no_grad():
            return mdl.head(mdl.forward_encoder(b)).view(1, 2, -1).clone()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        before = EvalGraph.for_model(mdl, batch)
        v0 = mdl.sf_mdl.eval_version
        assert before.captured_version == (v0, True)
        before.replay()
        uncal = before.feats.clone()
    side.synchronize()
    assert torch.equal(uncal, eager(batch))
    assert mdl.sf_mdl.eval_version == v0  # an eager forward with unchanged folds bumps nothing

    assert mdl.calibrate_weight_rounding(cal) > 0
    assert mdl.sf_mdl.eval_version > v0
    with torch.cuda.stream(side):
        with pytest.raises(_lib.VsError, match="stale eval graph"):
            before.replay()
        after = EvalGraph.for_model(mdl, batch)
        after.replay()
        got = after.feats.clone()
        after.inp.copy_(other["frms_ev_raw_u8"])  # the static input takes the next batch
        after.replay()
        got_other = after.feats.clone()
    side.synchronize()
    want = eager(batch)
    assert torch.equal(got, want)
    assert not torch.equal(want, uncal)  # the calibration does change the features: the stale graph would have been wrong
    assert torch.equal(got_other, eager(other))
    with torch.cuda.stream(side):
        with pytest.raises(_lib.VsError, match="stale eval graph"):
            before.replay()

    mdl.sf_mdl.reset_weight_rounding()
    with torch.cuda.stream(side):
        with pytest.raises(_lib.VsError, match="stale eval graph"):
            after.replay()
    side.synchronize()
    assert crop > 0
