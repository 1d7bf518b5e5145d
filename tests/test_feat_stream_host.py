"""Host-only side of the streaming feature extractor: the stand-in dataset's frame modes, the command line, the band
planner of the fused ingest kernel and the stale-graph check of `EvalGraph` (on a stub: no device)."""
import ctypes as C

import pytest
import torch

from vidsitu_amd import _lib, feat_extractor, ops, synth_data
from vidsitu_amd.eval_graph import EvalGraph
from vidsitu_amd.extended_config import get_cfg


def _cfg():
    cfg = get_cfg({"mdl.sf_mdl_name": "slow_fast_mini", "synth.num_verbs": 23})
    return cfg, synth_data.make_comm(cfg)


def test_synth_frame_dataset_modes():
    cfg, comm = _cfg()
    t = cfg.sf_mdl.DATA.NUM_FRAMES
    want = {"fp32": {"frms_ev_fast_tensor": ((2, 3, t, 32, 32), torch.float32),
                     "frms_ev_slow_tensor": ((2, 3, t // cfg.sf_mdl.SLOWFAST.ALPHA, 32, 32), torch.float32)},
            "u8": {"frms_ev_fast_u8": ((2, t, 32, 32, 3), torch.uint8)},
            "raw_u8": {"frms_ev_raw_u8": ((2, t, 45, 80, 3), torch.uint8)}}
    for mode, keys in want.items():
        ds = feat_extractor.SynthFrameDataset(cfg, comm, 3, n_ev=2, seed=7, crop=32, frames=mode, src_hw=(45, 80))
        assert len(ds) == 3
        a, b, other = ds[1], ds[1], ds[2]
        assert {k for k in a if k.startswith("frms_")} == set(keys), mode
        assert a["vseg_idx"].dtype == torch.int64 and int(a["vseg_idx"]) == 1
        for k, (shape, dtype) in keys.items():
            assert tuple(a[k].shape) == shape and a[k].dtype == dtype, (mode, k)
            assert torch.equal(a[k], b[k]), (mode, k)  # deterministic per index
            assert not torch.equal(a[k], other[k]), (mode, k)
    # the default is the fp32 contract, as before
    d = feat_extractor.SynthFrameDataset(cfg, comm, 1, n_ev=2, seed=7, crop=32)[0]
    assert "frms_ev_fast_tensor" in d and d["frms_ev_fast_tensor"].dtype == torch.float32
    with pytest.raises(ValueError):
        feat_extractor.SynthFrameDataset(cfg, comm, 1, frames="jpeg")


def test_u8_modes_draw_video_like_frames():
    """`synth_video_u8_batch` is the stand-in dataset's source (its docstring says so): the u8 item IS that batch."""
    cfg, comm = _cfg()
    ds = feat_extractor.SynthFrameDataset(cfg, comm, 2, n_ev=2, seed=3, crop=32, frames="u8")
    ref = synth_data.synth_video_u8_batch(cfg, comm, bs=1, n_ev=2, seed=3 + 1, crop=32)
    assert torch.equal(ds[1]["frms_ev_fast_u8"], ref["frms_ev_fast_u8"][0])
    raw = synth_data.synth_video_u8_batch(cfg, comm, bs=1, n_ev=2, seed=3, hw=(20, 36))
    assert tuple(raw["frms_ev_fast_u8"].shape[-3:]) == (20, 36, 3)


def test_argument_parsing():
    p = feat_extractor.parse_args
    w, n, kw = p(["weights.pth", "sfast"])
    assert (w, n) == ("weights.pth", "sfast") and kw == {"is_cu": False}  # main's defaults: fp32, no stream
    _, _, kw = p(["w", "n", "--frames=raw_u8", "--src_hw=256x340", "--stream=1", "--calibrate=0", "--is_cu=True",
                  "--splits=valid", "--train.bsv=2"])
    assert kw == {"frames": "raw_u8", "src_hw": (256, 340), "stream": 1, "calibrate": 0, "is_cu": True,
                  "splits": ("valid",), "train.bsv": "2"}
    assert p(["w", "n", "--frames=u8", "--stream=0"])[2] == {"frames": "u8", "stream": 0, "is_cu": False}
    for bad in (["w"], ["w", "n", "--frames=jpeg"], ["w", "n", "--src_hw=256"], ["w", "n", "--src_hw=0x4"],
                ["w", "n", "--stream=2"], ["w", "n", "--stream=1"], ["w", "n", "--frames=fp32", "--stream=1"],
                ["w", "n", "frames=u8"]):
        with pytest.raises(SystemExit):
            p(bad)
    import inspect

    sig = inspect.signature(feat_extractor.main).parameters
    assert sig["frames"].default == "fp32" and sig["stream"].default == 0 and sig["src_hw"].default == (256, 340)


def _bounds(in_size, out_size):
    lib = _lib.load()
    ks = lib.vs_resize_ksize(in_size, out_size)
    b = torch.zeros((out_size, 2), dtype=torch.int32)
    k = torch.zeros((out_size, ks), dtype=torch.int32)
    _lib.check(lib.vs_resize_coeffs(in_size, out_size, C.c_void_p(b.data_ptr()), C.c_void_p(k.data_ptr())), "coeffs")
    return b, ks


@pytest.mark.parametrize("budget", [64 * 1024, 48 * 1024, 24 * 1024])
@pytest.mark.parametrize("h0,ho,wo", [(360, 224, 224), (256, 224, 224), (240, 224, 224), (224, 224, 224),
                                      (100, 224, 224), (1080, 224, 224), (45, 64, 64), (33, 64, 16)])
def test_band_planner(h0, ho, wo, budget):
    band, rows, lds = ops.ingest_plan(h0, ho, wo, budget)
    assert 1 <= band <= 32 and lds <= budget
    pitch = (wo + 3) // 4 * 12
    assert pitch >= wo * 3
    ks = 0
    # every output row belongs to exactly one band, and the band's source rows fit the tile
    covered = []
    if h0 != ho:
        b, ks = _bounds(h0, ho)
    for y0 in range(0, ho, band):
        ys = list(range(y0, min(ho, y0 + band)))
        covered += ys
        if h0 != ho:
            lo = int(b[ys[0], 0])
            hi = max(int(b[y, 0] + b[y, 1]) for y in ys)
            assert min(int(b[y, 0]) for y in ys) == lo  # windows start in row order: the first row's is the lowest
            assert hi - lo <= rows, (y0, lo, hi, rows)
            assert 0 <= lo and hi <= h0
        else:
            assert len(ys) <= rows
    assert covered == list(range(ho))
    # the block's LDS: normalisation table + vertical weights and windows + tile
    assert lds == 3 * 256 * 2 + band * (ks + 2) * 4 + rows * pitch
    if band < min(32, ho):  # the largest band that fits: one row more would not
        rows1 = max((int(b[min(ho, y0 + band + 1) - 1, 0] + b[min(ho, y0 + band + 1) - 1, 1]) - int(b[y0, 0])
                     for y0 in range(0, ho, band + 1)), default=0) if h0 != ho else band + 1
        assert 3 * 256 * 2 + (band + 1) * (ks + 2) * 4 + rows1 * pitch > budget


def test_band_planner_sizes_of_the_issue():
    """360 -> 224 keeps 32-row bands well inside 64 KiB; 1080 -> 224 has to shrink the band to stay there."""
    band360, rows360, lds360 = ops.ingest_plan(360, 224, 224)
    band1080, rows1080, lds1080 = ops.ingest_plan(1080, 224, 224)
    assert band360 == 32 and lds360 <= 48 * 1024
    assert band1080 < 32 and lds1080 <= 64 * 1024
    with pytest.raises(_lib.VsError):
        ops.ingest_plan(1080, 224, 224, lds_budget=4096)  # not even one output row fits


class _StubGraph(EvalGraph):
    """The device halves replaced: `EvalGraph`'s version logic alone."""

    def __init__(self, trunk):
        super().__init__(step=lambda: None, version=lambda: trunk["v"])
        self.trunk, self.captures, self.replays = trunk, 0, 0

    def _capture(self):
        self.trunk["v"] += 1  # a warm-up's first forward re-folds: the recorded value must be the one AFTER it
        self.captures += 1
        return "out"

    def _replay(self):
        self.replays += 1


def test_eval_graph_refuses_a_stale_replay():
    trunk = {"v": 3}
    g = _StubGraph(trunk)
    with pytest.raises(_lib.VsError, match="before capture"):
        g.replay()
    g.capture()
    assert g.captured_version == 4
    assert g.replay() == "out" and g.replay() == "out" and g.replays == 2
    trunk["v"] += 1  # calibrate_weight_rounding / reset_weight_rounding / a re-fold
    with pytest.raises(_lib.VsError, match="stale eval graph.*calibrate_weight_rounding"):
        g.replay()
    with pytest.raises(_lib.VsError):
        g.replay()  # and stays refused
    assert g.replays == 2 and g.captures == 1  # never recaptured behind the caller's back
    g.capture()
    assert g.replay() == "out" and g.captures == 2 and g.replays == 3
