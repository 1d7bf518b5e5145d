"""Weight decay in `ArenaAdam`'s checkpoint state, and the schedule's state in the checkpoint file (no GPU): a
`torch.optim.AdamW` state and a `torch.optim.Adam(weight_decay=...)` state each load, select their form, and come back
out with the same `param_groups` values; `amsgrad` and unequal groups still raise."""
import pytest
import torch

from vidsitu_amd import checkpoint, lr_sched, synth_data
from vidsitu_amd.extended_config import get_cfg
from vidsitu_amd.mdl_selector import get_mdl_loss_eval
from vidsitu_amd.optim import ArenaAdam, ParamArena, reference_param_order


@pytest.fixture(scope="module")
def mdl():
    cfg = get_cfg({"mdl.sf_mdl_name": "i3d_tiny", "synth.num_verbs": 23})
    comm = synth_data.make_comm(cfg)
    torch.manual_seed(0)
    return get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=comm)


def _torch_state(mdl, cls, **kw):
    """Two steps of a stock optimizer over the reference model's parameter list (the upstream head that only the
    reference builds included: it never receives a gradient)."""
    shapes = checkpoint.reference_only_keys(mdl)
    index = reference_param_order(mdl)
    plist = [torch.nn.Parameter(torch.zeros(shapes[n]) if p is None else p.detach().clone().contiguous())
             for n, p in index]
    opt = cls(plist, lr=2e-4, betas=(0.9, 0.99), **kw)
    g = torch.Generator().manual_seed(1)
    for (_, p), q in zip(index, plist):
        if p is not None:
            q.grad = torch.randn(q.shape, generator=g)
    opt.step()
    opt.step()
    return plist, opt.state_dict()


@pytest.mark.parametrize("cls,decoupled", [(torch.optim.Adam, False), (torch.optim.AdamW, True)], ids=["Adam_L2", "AdamW"])
def test_torch_weight_decay_state_loads_and_comes_back(mdl, cls, decoupled):
    plist, sd = _torch_state(mdl, cls, weight_decay=0.05)
    assert sd["param_groups"][0].get("decoupled_weight_decay", False) is decoupled
    arena = ParamArena(mdl, adopt_conv=False)
    opt = ArenaAdam(arena, lr=3e-3)
    assert opt.hyper is None
    opt.load_state_dict(sd)
    assert opt.weight_decay == 0.05 and opt.decoupled_weight_decay is decoupled and opt.lr == 2e-4 and int(opt.t) == 2
    # the decay needs the device-side path: selected by the load, with the loaded values in the block
    assert opt.hyper is not None and torch.equal(opt.hyper[:3], torch.tensor([2e-4, 0.05, 0.0], dtype=torch.float32))
    back = opt.state_dict()
    g0, b0 = sd["param_groups"][0], back["param_groups"][0]
    for k in ("lr", "betas", "eps", "weight_decay", "decoupled_weight_decay", "amsgrad", "params"):
        assert b0[k] == g0[k] or tuple(b0[k]) == tuple(g0[k]), k
    stock = cls(plist, lr=1.0)
    stock.load_state_dict(back)
    assert stock.param_groups[0]["weight_decay"] == 0.05 and stock.param_groups[0]["lr"] == 2e-4
    assert stock.param_groups[0].get("decoupled_weight_decay", decoupled) is decoupled
    # an absent key means torch.optim.Adam's form
    legacy = {"state": sd["state"], "param_groups": [{k: v for k, v in g0.items() if k != "decoupled_weight_decay"}]}
    opt2 = ArenaAdam(arena, decoupled_weight_decay=True, weight_decay=0.5)
    opt2.load_state_dict(legacy)
    assert opt2.weight_decay == 0.05 and opt2.decoupled_weight_decay is False


def test_constructor_round_trip_and_the_default_group(mdl):
    arena = ParamArena(mdl, adopt_conv=False)
    plain = ArenaAdam(arena, lr=1e-4).state_dict()["param_groups"][0]
    assert plain["weight_decay"] == 0 and plain["decoupled_weight_decay"] is False and plain["amsgrad"] is False
    opt = ArenaAdam(arena, lr=1e-4, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0, dynamic_lr=True)
    g = opt.state_dict()["param_groups"][0]
    assert g["weight_decay"] == 0.01 and g["decoupled_weight_decay"] is True
    opt.set_lr(5e-5)
    assert opt.lr == 5e-5 and float(opt.hyper[0]) == float(torch.tensor(5e-5, dtype=torch.float32))
    assert opt.state_dict()["param_groups"][0]["lr"] == 5e-5
    with pytest.raises(ValueError):
        ArenaAdam(arena, weight_decay=-1.0)


def test_amsgrad_and_unequal_groups_still_raise(mdl):
    _, sd = _torch_state(mdl, torch.optim.Adam, amsgrad=True)
    opt = ArenaAdam(ParamArena(mdl, adopt_conv=False))
    with pytest.raises(ValueError, match="amsgrad"):
        opt.load_state_dict(sd)
    _, sd = _torch_state(mdl, torch.optim.AdamW, weight_decay=0.05)
    n = len(sd["param_groups"][0]["params"])
    g0 = sd["param_groups"][0]
    sd["param_groups"] = [dict(g0, params=list(range(n // 2))), dict(g0, params=list(range(n // 2, n)), weight_decay=0.0)]
    with pytest.raises(ValueError, match="groups"):
        opt.load_state_dict(sd)
    sd["param_groups"][1]["weight_decay"] = 0.05  # equal groups are one set of hyper-parameters
    opt.load_state_dict(sd)
    assert opt.weight_decay == 0.05 and opt.decoupled_weight_decay is True


def test_checkpoint_keeps_the_scheduler_state(mdl, tmp_path):
    arena = ParamArena(mdl, adopt_conv=False)
    opt = ArenaAdam(arena, lr=1e-3, dynamic_lr=True)
    sched = lr_sched.ReduceLROnPlateau(opt, factor=0.5, patience=0)
    for x in (3.0, 3.0, 2.0, 2.5):
        sched.step(x)
    assert opt.lr == 2.5e-4
    path = str(tmp_path / "models" / "ck.pth")
    ck = checkpoint.save_model_dict(path, mdl, opt, num_it=4, scheduler=sched)
    assert ck["scheduler_state_dict"] == sched.state_dict()
    opt2 = ArenaAdam(arena, lr=1e-3, dynamic_lr=True)
    sched2 = lr_sched.ReduceLROnPlateau(opt2, factor=0.9, patience=5)
    got = checkpoint.load_model_dict(path, mdl, opt2, load_opt=True, scheduler=sched2)
    assert got["num_it"] == 4 and opt2.lr == 2.5e-4 and float(opt2.hyper[0]) == float(torch.tensor(2.5e-4, dtype=torch.float32))
    assert sched2.state_dict() == sched.state_dict()
    assert sched2.get_last_lr()[0] == opt2.state_dict()["param_groups"][0]["lr"]
    # torch's own class accepts the saved state (the reference's trainer loads it: utils/trn_utils.py:704-706)
    stock = torch.optim.lr_scheduler.ReduceLROnPlateau(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=2.5e-4))
    stock.load_state_dict(torch.load(path, weights_only=True)["scheduler_state_dict"])
    assert stock.state_dict() == sched.state_dict()
    # without load_opt the schedule is left alone, and a file without the key loads as before
    sched3 = lr_sched.ReduceLROnPlateau(ArenaAdam(arena, lr=1e-3, dynamic_lr=True), factor=0.9, patience=5)
    before = sched3.state_dict()
    checkpoint.load_model_dict(path, mdl, None, load_opt=False, scheduler=sched3)
    assert sched3.state_dict() == before
    checkpoint.save_model_dict(path, mdl, opt, num_it=5)
    assert checkpoint.load_model_dict(path, mdl, opt2, load_opt=True, scheduler=sched3)["num_it"] == 5
    assert sched3.state_dict() == before
