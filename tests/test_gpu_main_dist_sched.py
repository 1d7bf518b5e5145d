"""`main_dist.py` with a schedule on hardware: warm-up per iteration, validation every two steps feeding
ReduceLROnPlateau, clipping inside the captured step; the checkpoint carries a `scheduler_state_dict` torch's own class
accepts, in step with the optimizer's rate, and a resumed run restores both.  One fresh child process per run."""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MINI = ["--mdl.sf_mdl_name=slow_fast_mini", "--sf_mdl.DATA.TRAIN_CROP_SIZE=64", "--synth.num_verbs=31",
        "--train.bs=2", "--ds.vsitu.num_ev=2", "--train.lr=1e-3", "--overfit_batch=True"]
SCHED = ["--val_every=2", "--train.use_reduce_lr_plateau=True", "--train.max_grad_norm=1.0", "--train.warmup_it=2"]


def _run(cmd, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    err = "\n".join(ln for ln in r.stderr.splitlines() if "frame #" not in ln)
    return r.returncode, r.stdout, err[-6000:]


def _load(path):
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert "scheduler_state_dict" in ck, sorted(ck)
    stock = torch.optim.lr_scheduler.ReduceLROnPlateau(
        torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0), factor=0.5, patience=3)
    stock.load_state_dict(ck["scheduler_state_dict"])  # torch's class accepts it
    assert set(ck["scheduler_state_dict"]) == set(stock.state_dict())
    return ck, stock


def test_main_dist_with_warmup_plateau_schedule_and_clipping(dev, tmp_path):
    args = ["main_dist.py", "t_sched"] + MINI + SCHED + [f"--misc.tmp_path={tmp_path}", "--steps=6"]
    rc, out, err = _run(args)
    assert rc == 0, out[-3000:] + err
    assert "hipGraph replay" in out, out
    m = re.search(r"loss ([-\d.e]+) -> ([-\d.e]+)", out)
    assert m and float(m.group(2)) < float(m.group(1)), out  # it trains: warm-up to 1e-3, clipped at norm 1
    ck, stock = _load(tmp_path / "models" / "t_sched.pth")
    group = ck["optimizer_state_dict"]["param_groups"][0]
    assert stock._last_lr[0] == group["lr"] == 1e-3  # the warm-up is over, the plateau schedule has not reduced yet
    assert stock.factor == 0.1 and stock.patience == 10 and stock.last_epoch == 2  # cfg.reduce_factor / cfg.patience; two validations
    assert ck["num_it"] == 6
    # resume: optimizer and schedule come back, and the rate is the restored one (no second warm-up)
    rc, out2, err = _run(args + ["--train.resume=True"])
    assert rc == 0, out2[-3000:] + err
    assert "resumed" in out2 and "at iteration 6, lr 0.001" in out2, out2
    ck2, stock2 = _load(tmp_path / "models" / "t_sched.pth")
    assert ck2["num_it"] == 12 and stock2.last_epoch == 4 and stock2.best <= stock.best
    assert stock2._last_lr[0] == ck2["optimizer_state_dict"]["param_groups"][0]["lr"] == 1e-3
