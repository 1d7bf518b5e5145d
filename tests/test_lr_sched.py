"""`vidsitu_amd.lr_sched` against torch's own schedulers (no GPU): the same metric sequence gives the same rates step
by step, and the state dicts load across the two implementations in both directions."""
import pytest
import torch

from vidsitu_amd import lr_sched

# improvement, a plateau longer than `patience`, a cooldown, further plateaus down to the `min_lr` floor
METRICS = ([5.0, 4.0, 3.0] + [3.0] * 4 + [3.5] * 3 + [2.0] + [2.5] * 12 + [2.4999] * 8)
PLATEAU_KW = [
    dict(mode="min", factor=0.1, patience=2, threshold=1e-4, threshold_mode="rel", cooldown=2, min_lr=3e-6, eps=1e-8),
    dict(mode="min", factor=0.5, patience=0, threshold=1e-2, threshold_mode="abs", cooldown=0, min_lr=1e-4, eps=1e-8),
    dict(mode="max", factor=0.3, patience=1, threshold=1e-3, threshold_mode="rel", cooldown=1, min_lr=0, eps=1e-8),
    dict(mode="max", factor=0.3, patience=3, threshold=0.1, threshold_mode="abs", cooldown=0, min_lr=0, eps=1e-5),
]


def _torch_opt(lr=1e-3):
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=lr)


class _Opt:
    """What the schedules need of an ArenaAdam."""

    def __init__(self, lr):
        self.lr, self.sets = lr, []

    def set_lr(self, x):
        self.lr = x
        self.sets.append(x)


def test_torch_refuses_an_arena_optimizer():
    with pytest.raises(TypeError):
        torch.optim.lr_scheduler.ReduceLROnPlateau(_Opt(1e-3))


@pytest.mark.parametrize("kw", PLATEAU_KW, ids=[f"{k['mode']}_{k['threshold_mode']}" for k in PLATEAU_KW])
def test_reduce_lr_on_plateau_follows_torch_step_by_step(kw):
    o_t, o_m, o_a = _torch_opt(), _torch_opt(), _Opt(1e-3)
    theirs = torch.optim.lr_scheduler.ReduceLROnPlateau(o_t, **kw)
    mine = lr_sched.ReduceLROnPlateau(o_m, **kw)
    arena = lr_sched.ReduceLROnPlateau(o_a, **kw)
    assert set(mine.state_dict()) == set(theirs.state_dict())
    sign = 1.0 if kw["mode"] == "min" else -1.0
    rates = []
    for x in METRICS:
        for s in (theirs, mine, arena):
            s.step(sign * x)
        rates.append(o_t.param_groups[0]["lr"])
        assert o_m.param_groups[0]["lr"] == rates[-1] and o_a.lr == rates[-1], (len(rates), rates[-1])
        assert mine.state_dict() == theirs.state_dict() == arena.state_dict()
    assert len(set(rates)) >= 3, rates  # the sequence did reduce more than once
    if kw["min_lr"] > 0:
        assert rates[-1] == kw["min_lr"], rates  # ... down to the floor
    assert o_a.sets == [r for prev, r in zip([1e-3] + rates, rates) if r != prev]  # set_lr only on a change


def test_plateau_state_crosses_over_in_both_directions():
    kw = PLATEAU_KW[0]
    half = len(METRICS) // 2
    o_t, o_m = _torch_opt(), _Opt(1e-3)
    theirs = torch.optim.lr_scheduler.ReduceLROnPlateau(o_t, **kw)
    mine = lr_sched.ReduceLROnPlateau(o_m, **kw)
    for x in METRICS[:half]:
        theirs.step(x)
        mine.step(x)
    # each continues from the other's state (fresh objects built with other settings)
    o_t2, o_m2 = _torch_opt(o_m.lr), _Opt(o_t.param_groups[0]["lr"])
    theirs2 = torch.optim.lr_scheduler.ReduceLROnPlateau(o_t2, mode="max", factor=0.9, patience=7)
    mine2 = lr_sched.ReduceLROnPlateau(o_m2, mode="max", factor=0.9, patience=7)
    theirs2.load_state_dict(mine.state_dict())
    mine2.load_state_dict(theirs.state_dict())
    for x in METRICS[half:]:
        for s in (theirs, mine, theirs2, mine2):
            s.step(x)
        want = o_t.param_groups[0]["lr"]
        assert o_m.lr == want and o_t2.param_groups[0]["lr"] == want and o_m2.lr == want
    assert theirs2.state_dict() == mine2.state_dict() == theirs.state_dict()


def test_lambda_lr_follows_torch_and_crosses_over():
    fn = lr_sched.warmup_linear(5, 40)
    o_t, o_m = _torch_opt(3e-4), _Opt(3e-4)
    theirs = torch.optim.lr_scheduler.LambdaLR(o_t, lr_sched.warmup_linear(5, 40))
    mine = lr_sched.LambdaLR(o_m, fn)
    assert set(mine.state_dict()) == set(theirs.state_dict())
    assert o_m.lr == o_t.param_groups[0]["lr"] == 3e-4 / 6  # construction applies fn(0)
    for _ in range(20):
        theirs.step()
        mine.step()
        assert o_m.lr == o_t.param_groups[0]["lr"]
    assert mine.state_dict() == theirs.state_dict()
    o_t2, o_m2 = _torch_opt(1.0), _Opt(1.0)
    theirs2 = torch.optim.lr_scheduler.LambdaLR(o_t2, lr_sched.warmup_linear(1, 2))
    mine2 = lr_sched.LambdaLR(o_m2, lr_sched.warmup_linear(1, 2))
    theirs2.load_state_dict(mine.state_dict())
    mine2.load_state_dict(theirs.state_dict())
    for _ in range(25):
        for s in (theirs, theirs2, mine2):
            s.step()
        want = o_t.param_groups[0]["lr"]
        assert o_t2.param_groups[0]["lr"] == want and o_m2.lr == want
    assert want == 0.0  # past total_it


def test_warmup_linear():
    fn = lr_sched.warmup_linear(3)
    assert [fn(i) for i in range(6)] == [0.25, 0.5, 0.75, 1.0, 1.0, 1.0]
    assert lr_sched.warmup_linear(0)(0) == 1.0
    decay = lr_sched.warmup_linear(2, 10)
    assert decay(2) == 1.0 and decay(6) == 0.5 and decay(10) == 0.0 and decay(11) == 0.0
