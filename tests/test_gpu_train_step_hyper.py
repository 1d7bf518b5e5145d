"""`TrainStep` with an `ArenaAdam` whose hyper-parameters live in device memory: a captured step follows `set_lr`,
clipping and weight decay replay exactly as they run eagerly, a rate that a capture froze is not silently ignored,
and the default optimizer still launches what it launched before.  Fixture of tests/test_gpu_train_step.py:
`slow_fast_mini`, 2-layer encoder without dropout, bs 2 x 2 events at crop 64."""
import gc
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

NORM_BOUND = 4 * 2.0 ** -24  # tests/test_gpu_adam_hyper.py


class _Calls:
    """Records the C-ABI entry points a wrapper goes through."""

    def __init__(self, monkeypatch, ops):
        self.names = []
        orig = ops._lib.call

        def call(name, *args):
            self.names.append(name)
            return orig(name, *args)

        monkeypatch.setattr(ops._lib, "call", call)


@pytest.fixture(scope="module")
def rig(dev):
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval
    from vidsitu_amd.optim import ParamArena

    cfg = get_cfg({"mdl.mdl_name": "sf_base_txenc", "mdl.sf_mdl_name": "slow_fast_mini", "synth.num_verbs": 31,
                   "tx_dec.encoder_layers": 2, "tx_dec.dropout": 0.0})
    comm = synth_data.make_comm(cfg)
    torch.manual_seed(0)
    sel = get_mdl_loss_eval(cfg)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev).train()
    loss_fn = sel["loss"](cfg, comm)
    arena = ParamArena(mdl)
    batch = synth_data.synth_batch(cfg, comm, bs=2, n_ev=2, crop=64, device=dev, dtype=torch.bfloat16)
    init = arena.data.clone()
    bufs = {k: v.clone() for k, v in mdl.named_buffers()}

    def reset(opt):
        arena.data.copy_(init)
        opt.m.zero_(); opt.v.zero_(); opt.t.zero_()
        for k, v in mdl.named_buffers():
            v.copy_(bufs[k])
        arena.refresh()
        torch.cuda.synchronize()

    return mdl, loss_fn, arena, batch, reset


def _eager(ts, steps):
    gc.collect()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(steps):
            ts.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_a_captured_step_follows_set_lr(rig):
    """Capture at lr 1e-3, replay, set_lr(0), replay: the second replay moves no parameter while the moments and the
    step count go on.  (With the rate as a launch argument the second replay would train on at 1e-3.)"""
    from vidsitu_amd.optim import ArenaAdam
    from vidsitu_amd.train_step import TrainStep

    mdl, loss_fn, arena, batch, reset = rig
    opt = ArenaAdam(arena, lr=1e-3, dynamic_lr=True)
    ts = TrainStep(mdl, loss_fn, arena, opt, batch, adam_overlap=False)
    reset(opt)
    _eager(ts, 1)
    ts.capture()
    reset(opt)
    p0 = arena.data.clone()
    ts.replay()
    torch.cuda.synchronize()
    p1, m1, v1 = arena.data.clone(), opt.m.clone(), opt.v.clone()
    assert int(opt.t) == 1 and not torch.equal(p1, p0)
    opt.set_lr(0.0)
    assert opt.lr == 0.0
    ts.replay()
    torch.cuda.synchronize()
    assert torch.equal(arena.data.view(torch.int32), p1.view(torch.int32)), "lr = 0 must leave every parameter as it is"
    assert int(opt.t) == 2 and not torch.equal(opt.m, m1) and not torch.equal(opt.v, v1)
    opt.set_lr(1e-3)
    ts.replay()
    torch.cuda.synchronize()
    assert not torch.equal(arena.data, p1) and int(opt.t) == 3


def test_clip_and_weight_decay_replay_as_they_run_eagerly(rig):
    from vidsitu_amd.optim import ArenaAdam
    from vidsitu_amd.train_step import TrainStep

    mdl, loss_fn, arena, batch, reset = rig
    # the norms of the two steps, measured by an armed clip that never bites
    probe = ArenaAdam(arena, lr=1e-3, weight_decay=0.01, max_grad_norm=1e9)
    ts = TrainStep(mdl, loss_fn, arena, probe, batch, adam_overlap=False)
    reset(probe)
    norms = []
    for i in range(2):
        _eager(ts, 1)
        norms.append(probe.last_grad_norm())
        assert probe.last_clip_coef() == 1.0 and norms[-1] > 0
        want = math.sqrt(float((arena.grad.double() ** 2).sum()))
        err = abs(norms[-1] - want) / want
        print(f"PARITY train_step grad_norm step {i} measured={norms[-1]:.7e} fp64={want:.7e} err={err:.3e} "
              f"bound={NORM_BOUND:.3e}")
        assert err <= NORM_BOUND

    limit = 0.1 * min(norms)  # (the first Adam step does not depend on the gradient's scale: the second norm stays close)
    opt = ArenaAdam(arena, lr=1e-3, weight_decay=0.01, max_grad_norm=limit)
    ts = TrainStep(mdl, loss_fn, arena, opt, batch, adam_overlap=False)

    def state():
        return [t.clone() for t in (arena.grad, arena.data, opt.m, opt.v, opt.t)]

    reset(opt)
    for i in range(2):
        _eager(ts, 1)
        want = math.sqrt(float((arena.grad.double() ** 2).sum()))
        err = abs(opt.last_grad_norm() - want) / want
        print(f"PARITY train_step grad_norm (clipped step {i}) norm={want:.7e} err={err:.3e} "
              f"coef={opt.last_clip_coef():.6f}")
        assert err <= NORM_BOUND and opt.last_clip_coef() < 1.0
    eager = state()
    ts.capture()
    reset(opt)
    ts.replay()
    ts.replay()
    torch.cuda.synchronize()
    replayed = state()
    assert int(replayed[4]) == 2
    for name, a, b in zip(("grad", "param", "exp_avg", "exp_avg_sq", "step"), eager, replayed):
        assert torch.equal(a, b), f"eager vs replayed {name} differs"


def test_a_rate_frozen_by_the_capture_is_not_silently_ignored(rig):
    from vidsitu_amd.optim import ArenaAdam
    from vidsitu_amd.train_step import TrainStep

    mdl, loss_fn, arena, batch, reset = rig
    opt = ArenaAdam(arena, lr=1e-3)
    ts = TrainStep(mdl, loss_fn, arena, opt, batch, adam_overlap=False)
    reset(opt)
    _eager(ts, 1)
    ts.capture()
    ts.replay()
    opt.lr = 1e-4
    with pytest.raises(RuntimeError, match="dynamic_lr"):
        ts.replay()
    with pytest.raises(RuntimeError):
        opt.set_lr(1e-4)
    opt.lr = 1e-3
    ts.replay()
    torch.cuda.synchronize()


def test_early_ranged_adam_refuses_clipping(rig):
    from vidsitu_amd.optim import ArenaAdam
    from vidsitu_amd.train_step import TrainStep

    mdl, loss_fn, arena, batch, _ = rig
    with pytest.raises(ValueError, match="max_grad_norm"):
        TrainStep(mdl, loss_fn, arena, ArenaAdam(arena, lr=1e-3, max_grad_norm=1.0), batch, adam_overlap=True)
    TrainStep(mdl, loss_fn, arena, ArenaAdam(arena, lr=1e-3), batch, adam_overlap=False)  # leaves the trunk un-deferred


def test_default_optimizer_goes_through_the_entry_points_it_always_did(rig, monkeypatch):
    """The names recorded on the parent commit: one fused launch per step, one per range after one tick; none of the
    device-side entry points, and no hyper block allocated."""
    from vidsitu_amd import ops
    from vidsitu_amd.optim import ArenaAdam

    mdl, loss_fn, arena, batch, reset = rig
    opt = ArenaAdam(arena, lr=1e-3)
    assert opt.hyper is None and opt.sumsq_ws is None
    reset(opt)
    arena.grad.normal_()
    calls = _Calls(monkeypatch, ops)
    opt.step()
    adam = [n for n in calls.names if "adam" in n or "sumsq" in n]
    assert adam == ["vs_adam_step_dev_cast"], calls.names
    del calls.names[:]
    opt.tick()
    opt.step_range(0, 1024)
    opt.step_range(1024, arena.numel)
    adam = [n for n in calls.names if "adam" in n or "sumsq" in n]
    assert adam == ["vs_adam_tick", "vs_adam_step_dev_range", "vs_adam_step_dev_range"], calls.names
    del calls.names[:]
    hp = ArenaAdam(arena, lr=1e-3, max_grad_norm=1.0)
    reset(hp)
    hp.step()
    adam = [n for n in calls.names if "adam" in n or "sumsq" in n]
    assert adam == ["vs_grad_sumsq", "vs_adam_step_hp"], calls.names
    whole = [t.clone() for t in (arena.data, hp.m, hp.v, hp.t, hp.hyper)]
    # the ranged form of the same optimizer: one norm pass over the whole arena before the first range, same bits
    del calls.names[:]
    reset(hp)
    hp.tick()
    hp.step_range(0, 1024)
    hp.step_range(1024, arena.numel)
    adam = [n for n in calls.names if "adam" in n or "sumsq" in n]
    assert adam == ["vs_adam_tick", "vs_grad_sumsq", "vs_adam_step_hp", "vs_adam_step_hp"], calls.names
    for a, b in zip(whole, (arena.data, hp.m, hp.v, hp.t, hp.hyper)):
        assert torch.equal(a, b)
    assert hp.last_clip_coef() < 1.0
    torch.cuda.synchronize()
