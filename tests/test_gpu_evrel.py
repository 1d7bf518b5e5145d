"""The event-relation task on the GPU: the RoBERTa encoder against the huggingface goldens, each of the five models
(logits, loss, every gradient) against the fp64 restatement of tests/roberta_ref.py, the training step, the evaluation
records and the `main_dist.py` entry point.  No transformers import, no reference import.

Bounds (those of tests/test_gpu_gpt2.py): outputs within 1e-3 of the reference's largest entry, the loss within 1e-4,
every parameter gradient within 5e-4 of that parameter's largest entry.  A parameter whose gradient is analytically
zero (`key.bias`: a shift of every key by one vector moves all scores of a query alike, which the softmax does not see;
both sides hold rounding noise) is compared on the scale of the largest gradient entry of the whole model instead.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import roberta_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
OUT_TOL, LOSS_TOL, GRAD_TOL = 1e-3, 1e-4, 5e-4


def _gold(name):
    return {k: v for k, v in np.load(os.path.join(GOLD, name)).items()}


def _rel(got, want):
    want = torch.as_tensor(want).double()
    return float((got.detach().cpu().double() - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def _check_grads(named_got, want, what):
    """named_got: {name: tensor | None}; want: {name: fp64 tensor}."""
    top = max(float(v.abs().max()) for v in want.values())
    worst = ("", 0.0)
    for k, w in want.items():
        g = named_got[k]
        assert g is not None and tuple(g.shape) == tuple(w.shape), k
        assert bool(torch.isfinite(g).all()), k
        scale = top if k.endswith("attention.self.key.bias") else float(w.abs().max())
        assert scale > 0, k
        err = float((g.detach().cpu().double() - w).abs().max()) / scale
        if err > worst[1]:
            worst = (k, err)
    print(f"PARITY {what}: worst gradient error {worst[1]:.3e} ({worst[0]}), largest entry {top:.3e}")
    assert worst[1] < GRAD_TOL, f"{what}: {worst[0]} {worst[1]:.3e}"


def _hip_models(dims, seed, dev):
    from vidsitu_amd.hf_roberta import RobertaForSequenceClassificationHip, RobertaModelHip

    m = RobertaModelHip(**dims).to(dev)
    m.load_state_dict({k: v.float() for k, v in ref.make_weights(dims, seed).items()})
    mc = RobertaForSequenceClassificationHip(**dims, num_labels=5).to(dev)
    wc = ref.make_weights(dims, seed, prefix="roberta.", pooler=False, num_labels=5)
    mc.load_state_dict({k: v.float() for k, v in wc.items()})
    return m, mc


def test_encoder_matches_the_tiny_golden_and_its_gradients(dev):
    """2 layers, 64 wide, 6 x 60, right padding down to 3 tokens: hidden state, pooler output, logits, and the
    5-label cross-entropy loss with every parameter gradient of the manual backward."""
    from vidsitu_amd import hf_roberta
    from vidsitu_amd.mdl_sf_base import hip_cross_entropy

    g, gg = _gold("roberta_tiny.npz"), _gold("roberta_tiny_grads.npz")
    toks, mask = torch.from_numpy(g["tokens"]).to(dev), torch.from_numpy(g["mask"]).to(dev)
    m, mc = _hip_models(ref.TINY, 21, dev)
    out = m.eval()(toks, mask)
    e = (_rel(out.last_hidden_state, g["hidden_states"][-1]), _rel(out.pooler_output, g["pooler_output"]),
         _rel(mc.eval()(toks, mask).logits, g["logits"]))
    print(f"PARITY roberta tiny golden: hidden {e[0]:.3e} pooler {e[1]:.3e} logits {e[2]:.3e}")
    assert max(e) < OUT_TOL
    mc.train()
    (logits,) = hf_roberta.roberta_apply(mc, toks, mask)
    assert logits.requires_grad
    loss = hip_cross_entropy(logits, torch.from_numpy(gg["labels"]).to(dev))
    loss.backward()
    print(f"PARITY roberta tiny golden: loss {float(loss.detach()):.6f} vs {float(gg['loss']):.6f}")
    assert abs(float(loss.detach()) - float(gg["loss"])) < LOSS_TOL * max(1.0, abs(float(gg["loss"])))
    want = {k[5:]: torch.from_numpy(v) for k, v in gg.items() if k.startswith("grad.")}
    _check_grads({k: mc.P(k).grad for k in want}, want, "roberta tiny golden")
    pad = ref.TINY["pad_token_id"]
    assert float(mc.P("roberta.embeddings.word_embeddings.weight").grad[pad].abs().max()) == 0.0
    assert float(mc.P("roberta.embeddings.position_embeddings.weight").grad[pad].abs().max()) == 0.0


def test_encoder_matches_the_wide_golden(dev):
    """A 2-layer slice of roberta-base's shape (768 wide, 12 heads of 64) at 3 x 120."""
    g = _gold("roberta_wide.npz")
    toks, mask = torch.from_numpy(g["tokens"]).to(dev), torch.from_numpy(g["mask"]).to(dev)
    m, mc = _hip_models(ref.WIDE, 22, dev)
    out = m.eval()(toks, mask)
    e = (_rel(out.last_hidden_state[:, ::2], g["last_hidden_even"]), _rel(out.pooler_output, g["pooler_output"]),
         _rel(mc.eval()(toks, mask).logits, g["logits"]))
    print(f"PARITY roberta wide golden: hidden {e[0]:.3e} pooler {e[1]:.3e} logits {e[2]:.3e}")
    assert max(e) < OUT_TOL


def test_all_zero_mask_row_and_missing_mask(dev):
    """A sequence whose mask is all zero (against the restatement only: newer huggingface releases differ), and no
    mask at all."""
    g = _gold("roberta_tiny.npz")
    toks, mask = torch.from_numpy(g["tokens"]), torch.from_numpy(g["mask"]).clone()
    mask[2] = 0
    w = ref.make_weights(ref.TINY, 21)
    m, _ = _hip_models(ref.TINY, 21, dev)
    m.eval()
    for mk in (mask, None):
        h64 = ref.encoder(w, toks, mk, ref.TINY)
        out = m(toks.to(dev), None if mk is None else mk.to(dev))
        e = (_rel(out.last_hidden_state, h64), _rel(out.pooler_output, ref.pooler(w, h64)))
        print(f"PARITY roberta tiny {'zero-row mask' if mk is not None else 'no mask'}: hidden {e[0]:.3e} pooler {e[1]:.3e}")
        assert max(e) < OUT_TOL


def _close(a, b):
    # the embedding backward accumulates rows with atomics: equal up to fp32 summation order
    return bool(((a - b).abs().max() <= 1e-5 * a.abs().max().clamp_min(1e-12)).item())


@pytest.mark.parametrize("both", [True, False], ids=["both_outputs", "pooler_only"])
def test_two_forwards_keep_their_own_state(both, dev):
    """Two forwards on different inputs through `roberta_apply`, then the backwards in the opposite order: every
    parameter gradient equals that of each forward-backward pair run alone.  3 x 9 tokens, one row's tail masked;
    with a loss on `pooler_output` alone the hidden state's gradient reaches the node as None."""
    from vidsitu_amd import hf_roberta

    torch.manual_seed(5)
    m = hf_roberta.build("roberta-synth-tiny", hf_roberta.RobertaModelHip).to(dev).train()
    pad, d = m.pad, m.d_model
    g = torch.Generator().manual_seed(6)
    toks = [torch.randint(2, 101, (3, 9), generator=g) for _ in range(2)]
    toks[0][2, 5:] = pad
    toks[1][0, 7:] = pad
    toks = [t.to(dev) for t in toks]
    masks = [t.ne(pad) for t in toks]
    wh = [torch.randn(3, 9, d, generator=g).to(dev) for _ in range(2)]
    wp = [torch.randn(3, d, generator=g).to(dev) for _ in range(2)]
    for p in m.parameters():
        p.grad = torch.zeros_like(p)

    def run(i, scale):
        hidden, pooled = hf_roberta.roberta_apply(m, toks[i], masks[i])
        loss = (pooled * wp[i]).sum()
        if both:
            loss = loss + (hidden * wh[i]).sum()
        return loss * scale

    def grads(loss):
        for p in m.parameters():
            p.grad.zero_()
        loss.backward()
        return [p.grad.clone() for p in m.parameters()]

    want = [grads(run(i, 1.0 + i)) for i in range(2)]
    assert all(float(w.abs().max()) > 0 for w in want[0])
    la, lb = run(0, 1.0), run(1, 2.0)
    got_b = grads(lb)
    got_a = grads(la)
    for want_i, got_i in ((want[0], got_a), (want[1], got_b)):
        for n, w, gt in zip(m._names, want_i, got_i):
            assert _close(w, gt), n


# ---- the five models ------------------------------------------------------------------------------------------------
def _cfg(row):
    from vidsitu_amd.extended_config import get_cfg

    return get_cfg({"task_type": "evrel", "mdl.mdl_name": row, "mdl.rob_mdl_name": "roberta-synth-tiny"})


@functools.lru_cache(maxsize=None)
def _case(row, n_ann):
    """cfg, comm, batch (cpu), fp64 weights and the fp64 restatement's logits / loss / gradients: computed once."""
    from vidsitu_amd import synth_data
    from vidsitu_amd.hf_roberta import ROBERTA_DIMS
    from vidsitu_amd.mdl_sf_base import get_head_dim

    cfg = _cfg(row)
    comm = synth_data.make_comm(cfg)
    dims = ROBERTA_DIMS["roberta-synth-tiny"]
    head_dim = get_head_dim(cfg)
    batch = synth_data.synth_evrel_batch(comm, 2, n_ann=n_ann, feat_dim=head_dim, seed=40 + n_ann)
    w = ref.make_evrel_weights(row, dims, head_dim, 50 + n_ann)
    out64, loss64, g64 = ref.evrel_loss_and_grads(row, w, batch, dims)
    return cfg, comm, batch, w, out64, loss64, g64


def _build(row, n_ann, dev):
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    cfg, comm, batch, w, out64, loss64, g64 = _case(row, n_ann)
    sel = get_mdl_loss_eval(cfg)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev)
    mdl.load_state_dict({k: v.float() for k, v in w.items()}, strict=True)
    return sel, mdl, {k: v.to(dev) for k, v in batch.items()}


@pytest.mark.parametrize("n_ann", [1, 3])
@pytest.mark.parametrize("row", ref.EVREL_NAMES)
def test_evrel_model_against_fp64(row, n_ann, dev):
    """Logits, loss and every gradient at B = 2; the branch the reference multiplies out is not launched and leaves
    its parameters' grad None; eval mode gives the same logits as the training pass."""
    cfg, comm, batch, w, out64, loss64, g64 = _case(row, n_ann)
    sel, mdl, batch_d = _build(row, n_ann, dev)
    mdl.train()
    out = mdl(batch_d)
    loss = sel["loss"](cfg, comm)(out, batch_d)["loss"]
    assert tuple(out["mdl_out"].shape) == (2, 4, n_ann, 5) and loss.requires_grad
    loss.backward()
    e = _rel(out["mdl_out"], out64)
    print(f"PARITY {row} n_ann{n_ann}: logits {e:.3e}, loss {float(loss.detach()):.6f} vs {float(loss64):.6f}")
    assert e < OUT_TOL
    assert abs(float(loss.detach()) - float(loss64)) < LOSS_TOL * max(1.0, abs(float(loss64)))
    got = {k: v.grad for k, v in mdl.state_dict(keep_vars=True).items()}
    dead = {"txe_evrel": "vid_feat_encoder.", "sfpret_onlyvid_evrel": "rob_mdl."}.get(row)
    live = {k: v for k, v in g64.items() if not (dead and k.startswith(dead))}
    assert all(v is not None for v in live.values())
    if dead:
        skipped = [k for k in g64 if k.startswith(dead)]
        assert skipped and all(got[k] is None for k in skipped), "a skipped branch must leave grad None"
        assert all(g64[k] is None or float(g64[k].abs().max()) == 0.0 for k in skipped)
    _check_grads(got, live, f"{row} n_ann{n_ann}")
    mdl.eval()
    with torch.no_grad():
        ev = mdl(batch_d)
    assert torch.equal(ev["mdl_out"], out["mdl_out"]) and not ev["mdl_out"].requires_grad


@pytest.mark.parametrize("row", ["rob_evrel", "sfpret_evrel"])
def test_evrel_training_step_lowers_the_loss(row, dev):
    """20 Adam steps on one batch through the parameter arena."""
    from vidsitu_amd.optim import ArenaAdam, ParamArena

    cfg, comm, *_ = _case(row, 1)
    sel, mdl, batch_d = _build(row, 1, dev)
    mdl.train()
    loss_fn = sel["loss"](cfg, comm)
    arena = ParamArena(mdl, adopt_conv=False)
    opt = ArenaAdam(arena, lr=1e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = loss_fn(mdl(batch_d), batch_d)["loss"]
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print(f"{row}: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] - 0.05, losses


def test_evalb_acc_records(dev):
    """`EvalB_Acc.forward_one_batch`: per video 4 lists of n_ann relation names / probabilities and the video's
    index; `forward`: mean loss, Top_1 and Macro_Top_1 over the batch labels."""
    cfg, comm, batch, w, out64, loss64, _ = _case("sfpret_evrel", 3)
    sel, mdl, batch_d = _build("sfpret_evrel", 3, dev)
    evl = sel["evl"](cfg, comm, dev)
    assert evl.met_keys == ["Macro_Top_1", "Top_1"]
    recs = evl.forward_one_batch(mdl.eval(), batch_d)
    p64 = torch.softmax(out64, dim=-1)
    assert len(recs) == 2
    for b, rec in enumerate(recs):
        assert set(rec) == {"pred_evrels_ev", "pred_scores_ev", "ann_idx"} and rec["ann_idx"] == b
        assert len(rec["pred_evrels_ev"]) == len(rec["pred_scores_ev"]) == 4
        for e in range(4):
            assert len(rec["pred_evrels_ev"][e]) == len(rec["pred_scores_ev"][e]) == 3
            for a in range(3):
                top = int(p64[b, e, a].argmax())
                assert rec["pred_evrels_ev"][e][a] == comm.evrel_dct_opp[top]
                assert abs(rec["pred_scores_ev"][e][a] - float(p64[b, e, a, top])) < 1e-4
    loss_d, acc_d = evl(mdl, sel["loss"](cfg, comm), [batch_d])
    lab, pred = batch["evrel_labs"].reshape(-1), p64.argmax(-1).reshape(-1)
    per_cls = [float((pred[lab == c] == c).double().mean()) for c in lab.unique().tolist()]
    assert abs(loss_d["loss"] - float(loss64)) < LOSS_TOL * max(1.0, float(loss64))
    assert abs(acc_d["Top_1"] - float((pred == lab).double().mean())) < 1e-12
    assert abs(acc_d["Macro_Top_1"] - sum(per_cls) / len(per_cls)) < 1e-12


def test_main_dist_trains_sfpret_evrel(dev, tmp_path):
    """`main_dist.py <uid> --task_type=evrel ...`: three eager steps on the tiny encoder, validation, checkpoint."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    cmd = [sys.executable, "main_dist.py", "t_evrel", "--task_type=evrel", "--mdl.mdl_name=sfpret_evrel",
           "--mdl.rob_mdl_name=roberta-synth-tiny", "--train.bs=2", "--train.lr=1e-3", "--overfit_batch=True",
           f"--misc.tmp_path={tmp_path}", "--steps=3", "--num_gpus=1"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"loss ([-\d.e]+) -> ([-\d.e]+)", r.stdout)
    assert m and "(eager" in r.stdout, r.stdout
    assert float(m.group(2)) < float(m.group(1)), r.stdout
    assert "Macro_Top_1" in r.stdout and (tmp_path / "models" / "t_evrel.pth").exists()
