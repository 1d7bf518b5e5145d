"""Learning-rate schedules for `ArenaAdam` (host only).

torch's schedulers refuse anything that is not a `torch.optim.Optimizer` (TypeError), and `ArenaAdam` keeps one flat
arena, not `param_groups`.  The two schedules the reference trainer uses (`utils/trn_utils.py:896-912`:
`ReduceLROnPlateau` on the validation metric, `LambdaLR` for warm-up) are restated here with torch's arithmetic and
torch's `state_dict()` key set, so that a reference checkpoint's `scheduler_state_dict` loads here and one written
here loads into torch's class.  They drive `opt.set_lr(x)`: on an `ArenaAdam(dynamic_lr=True)` that is one fill of a
device float, which the captured step reads at its next replay.

An optimizer is anything with a readable `lr` and a `set_lr(x)`; a `torch.optim.Optimizer` is accepted too (its
first group is driven), which is how tests/test_lr_sched.py runs both implementations side by side.
"""
import math
import types


def _get_lr(opt):
    if hasattr(opt, "param_groups"):
        return opt.param_groups[0]["lr"]
    return opt.lr


def _set_lr(opt, x):
    if hasattr(opt, "param_groups"):
        for g in opt.param_groups:
            g["lr"] = x
    else:
        opt.set_lr(x)


class ReduceLROnPlateau:
    """`torch.optim.lr_scheduler.ReduceLROnPlateau` for one rate: `step(metric)` after every validation."""

    def __init__(self, optimizer, mode="min", factor=0.1, patience=10, threshold=1e-4, threshold_mode="rel",
                 cooldown=0, min_lr=0, eps=1e-8):
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        self.factor = factor
        self.optimizer = optimizer
        if isinstance(min_lr, (list, tuple)):
            if len(min_lr) != 1:
                raise ValueError(f"expected 1 min_lrs, got {len(min_lr)}")
            self.default_min_lr = None
            self.min_lrs = list(min_lr)
        else:
            self.default_min_lr = min_lr
            self.min_lrs = [min_lr]
        self.patience = patience
        self.cooldown = cooldown
        self.eps = eps
        self.last_epoch = 0
        self._last_lr = [_get_lr(optimizer)]
        self._init_is_better(mode, threshold, threshold_mode)
        self.best = self.mode_worse
        self.cooldown_counter = 0
        self.num_bad_epochs = 0

    def _init_is_better(self, mode, threshold, threshold_mode):
        if mode not in ("min", "max"):
            raise ValueError("mode " + mode + " is unknown!")
        if threshold_mode not in ("rel", "abs"):
            raise ValueError("threshold mode " + threshold_mode + " is unknown!")
        self.mode_worse = math.inf if mode == "min" else -math.inf
        self.mode, self.threshold, self.threshold_mode = mode, threshold, threshold_mode

    def _is_better(self, a, best):
        if self.mode == "min" and self.threshold_mode == "rel":
            return a < best * (1.0 - self.threshold)
        if self.mode == "min":
            return a < best - self.threshold
        if self.threshold_mode == "rel":
            return a > best * (self.threshold + 1.0)
        return a > best + self.threshold

    @property
    def in_cooldown(self):
        return self.cooldown_counter > 0

    def step(self, metrics):
        current = float(metrics)
        self.last_epoch += 1
        if self._is_better(current, self.best):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.in_cooldown:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0  # bad epochs in cooldown do not count
        if self.num_bad_epochs > self.patience:
            old_lr = float(_get_lr(self.optimizer))
            new_lr = max(old_lr * self.factor, self.min_lrs[0])
            if old_lr - new_lr > self.eps:
                _set_lr(self.optimizer, new_lr)
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0
        self._last_lr = [_get_lr(self.optimizer)]

    def get_last_lr(self):
        return self._last_lr

    def state_dict(self):
        return {k: v for k, v in self.__dict__.items() if k != "optimizer"}

    def load_state_dict(self, state_dict):
        self.__dict__.update(state_dict)
        self._init_is_better(self.mode, self.threshold, self.threshold_mode)
        if len(self.min_lrs) != 1 or len(self._last_lr) != 1:
            raise ValueError("scheduler state of more than one parameter group: one rate for the whole arena here")


class LambdaLR:
    """`torch.optim.lr_scheduler.LambdaLR` for one rate: lr = base_lr * fn(number of `step()` calls so far).
    Like torch's, construction applies fn(0)."""

    def __init__(self, optimizer, lr_lambda, last_epoch=-1):
        self.optimizer = optimizer
        self.lr_lambdas = [lr_lambda]
        self.base_lrs = [_get_lr(optimizer)]
        self.last_epoch = last_epoch
        self._step_count = 0
        self._is_initial = False
        self._get_lr_called_within_step = False
        self._last_lr = list(self.base_lrs)
        self.step()

    def step(self):
        self._step_count += 1
        self.last_epoch += 1
        lr = self.base_lrs[0] * self.lr_lambdas[0](self.last_epoch)
        _set_lr(self.optimizer, lr)
        self._last_lr = [_get_lr(self.optimizer)]

    def get_last_lr(self):
        return self._last_lr

    def state_dict(self):
        sd = {k: v for k, v in self.__dict__.items() if k not in ("optimizer", "lr_lambdas")}
        sd["lr_lambdas"] = [None if isinstance(fn, types.FunctionType) else fn.__dict__.copy()
                            for fn in self.lr_lambdas]
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        lr_lambdas = state_dict.pop("lr_lambdas")
        if len(lr_lambdas) != 1:
            raise ValueError("scheduler state of more than one parameter group: one rate for the whole arena here")
        self.__dict__.update(state_dict)
        if lr_lambdas[0] is not None:
            self.lr_lambdas[0].__dict__.update(lr_lambdas[0])


class warmup_linear:
    """Multiplier of a linear warm-up over `warmup_it` steps, then (with `total_it`) a linear decay to zero at
    `total_it`; without `total_it` the rate stays at its base after the warm-up.  A callable object, not a closure, so
    that `LambdaLR.state_dict()` carries its two numbers."""

    def __init__(self, warmup_it, total_it=None):
        self.warmup_it, self.total_it = int(warmup_it), (int(total_it) if total_it else None)

    def __call__(self, it):
        if self.warmup_it > 0 and it < self.warmup_it:
            return (it + 1) / (self.warmup_it + 1)
        if self.total_it is None:
            return 1.0
        return max(0.0, (self.total_it - it) / max(1, self.total_it - self.warmup_it))
