"""`GPT2LMHeadModelHip(..., matmul="bf16")`: bf16 operands with fp32 accumulation in the dense projections of the
whole-sequence passes, fp32 everywhere else, the default untouched.

gpt2-synth-tiny with the weights of `gpt2_ref.make_weights(97, 64, 64, 2, 23)`; R = 3, L = 23 (69 tokens: the dW GEMMs
have K % 4 != 0), one right-padded row, eight label sets -- the batch of tests/test_gpu_gpt2_dropout.py at another L.

Every call, tightly: `ops.gemm_nt` is wrapped for one bf16-mode forward_train + backward and one forward_logits; every
call's own recorded operands go through the restatement of tests/test_gpu_gemm_bf16.py (operands rounded with
`tensor.bfloat16()`, fp64, `e32` = the same in fp32) under the rule err <= min(16 * e32, 2e-4).  This is the tight
whole-model check: an end result cannot be held tightly to a restatement that rounds at every GEMM, because an
activation that lands on the other side of a bf16 rounding boundary moves the result by far more than fp32 noise.

End to end, loosely: `d_ref` = the fp64 deviation of tests/gpt2_bf16_ref.py (dense layers that round x, W and dy to
bf16) from the exact fp64 model, relative to max |exact|, computed here for the logits, the loss vector and every
parameter gradient.  The model's deviation from the exact fp64 model must be at most 2 * d_ref for every quantity and
at least d_ref / 2 for the logits (the mode is really on).  Every figure is printed (`PARITY ...`) before it is
asserted."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import gpt2_bf16_ref as bref
import gpt2_dropout_ref as gref
from oracle import gpt2_ref
from test_gpu_gemm_bf16 import ACT_NAMES, _restate
from test_gpu_gpt2_ops import CEILING, FACTOR, _bits, _errs, _gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LAYER, D, N_HEAD, N_POS, VOCAB = 2, 64, 4, 64, 97
PAD = VOCAB - 1
R, L = 3, 23
N_LABEL_SETS = 8
GEMMS_FWD = 4 * N_LAYER + 1      # c_attn, attn.c_proj, c_fc, mlp.c_proj per layer + the tied lm_head
GEMMS_BWD = 2 * GEMMS_FWD        # dW and dx of each


@functools.lru_cache(maxsize=None)
def _weights():
    return {k: torch.from_numpy(v) for k, v in gpt2_ref.make_weights(VOCAB, N_POS, D, N_LAYER, 23).items()}


@functools.lru_cache(maxsize=None)
def _batch():
    g = _gen(77)
    toks = torch.randint(0, PAD, (R, L), generator=g)
    toks[1, L - 5:] = PAD  # one right-padded row
    labels = [toks] + [torch.where(toks == PAD, toks, torch.randint(0, PAD, (R, L), generator=g))
                       for _ in range(N_LABEL_SETS - 1)]
    return toks, labels


def _model(dev, **kw):
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip

    m = GPT2LMHeadModelHip(N_LAYER, D, N_HEAD, N_POS, VOCAB, **kw)
    sd = dict(_weights())
    sd["lm_head.weight"] = sd["transformer.wte.weight"]
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def _train_pass(m, toks_d):
    from vidsitu_amd.hf_gpt2_fseq import _GPT2TrainFn

    tick = torch.zeros(1, device=toks_d.device, requires_grad=True)
    return _GPT2TrainFn.apply(m, toks_d, toks_d.ne(PAD), tick)


def _grads_after(m, toks_d):
    from vidsitu_amd.hf_gpt2_fseq import lm_loss

    for p in m.parameters():
        p.grad = None
    logits = _train_pass(m, toks_d)
    loss = lm_loss(logits, toks_d, PAD)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), loss.detach().clone(), {k: m.P(k).grad.clone() for k in m._names}


# ---------------------------------------------------------------------------------------------
# every GEMM call of the mode, each against the restatement from its own operands
# ---------------------------------------------------------------------------------------------
def _recording(monkeypatch):
    from vidsitu_amd import ops

    calls, real = [], ops.gemm_nt

    def gemm_nt(x, w, b=None, res=None, act=ops.ACT_NONE, out=None, bf16=False):
        rec = dict(x=x.detach().cpu().clone(), w=w.detach().cpu().clone(), b=None if b is None else b.detach().cpu().clone(),
                   res=None if res is None else res.detach().cpu().clone(), act=int(act), bf16=bf16)
        y = real(x, w, b, res, act=act, out=out, bf16=bf16)
        rec["y"] = y.detach().cpu().clone()
        calls.append(rec)
        return y

    monkeypatch.setattr(ops, "gemm_nt", gemm_nt)
    return calls


def _check_calls(name, calls):
    for i, c in enumerate(calls):
        assert c["bf16"] is True, f"{name}: call {i} ran with fp32 operands"
        (m, k), n = c["x"].shape, c["w"].shape[0]
        ref64 = _restate(c["x"], c["w"], c["b"], c["res"], c["act"], torch.float64)
        ref32 = _restate(c["x"], c["w"], c["b"], c["res"], c["act"], torch.float32)
        e32, err = _errs(c["y"], ref64, ref32)
        tag = f"{name} call {i} M={m} N={n} K={k} act={ACT_NAMES[c['act']]}" + (" bias" if c["b"] is not None else "") + (
            " res" if c["res"] is not None else "")
        print(f"PARITY {tag} e32={e32:.3e} err={err:.3e}")
        assert bool(torch.isfinite(c["y"]).all()), tag
        assert err <= min(FACTOR * e32, CEILING), f"{tag}: kernel error {err:.3e} vs fp32 floor {e32:.3e}"


def test_every_gemm_of_a_training_pass_takes_bf16_operands_and_matches_its_restatement(dev, monkeypatch):
    from vidsitu_amd.hf_gpt2_fseq import lm_loss

    m = _model(dev, matmul="bf16").train()
    toks, _ = _batch()
    td = toks.to(dev)
    calls = _recording(monkeypatch)
    logits = _train_pass(m, td)
    assert len(calls) == GEMMS_FWD
    lm_loss(logits, td, PAD).backward()
    assert len(calls) == GEMMS_FWD + GEMMS_BWD
    ks = sorted({c["x"].shape[1] for c in calls[GEMMS_FWD:]})
    assert R * L in ks and (R * L) % 4 != 0, "the dW GEMMs sum over the 69 tokens"
    _check_calls("gpt2 bf16 train", calls)


def test_every_gemm_of_forward_logits_takes_bf16_operands_and_none_of_the_decode_step_does(dev, monkeypatch):
    from vidsitu_amd.hf_gpt2_fseq import KVCacheState

    m = _model(dev, matmul="bf16").eval()
    toks, _ = _batch()
    td = toks.to(dev)
    calls = _recording(monkeypatch)
    m.forward_logits(td, td.ne(PAD))
    assert len(calls) == GEMMS_FWD
    assert sorted({c["act"] for c in calls}) == [0, 2]  # the gelu epilogue runs in this pass
    _check_calls("gpt2 bf16 forward_logits", calls)
    del calls[:]
    st = KVCacheState()
    for t in range(2):
        m.forward_step(td[:, t].contiguous(), st, max_len=8)
    assert len(calls) == 2 * GEMMS_FWD and all(c["bf16"] is False for c in calls)


# ---------------------------------------------------------------------------------------------
# end to end against the rounding restatement
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _refs():
    toks, labels = _batch()
    key_mask = toks.ne(PAD)
    exact = gref.run(_weights(), toks, key_mask, N_LAYER, N_HEAD, {}, PAD, labels, torch.float64)
    rounded = bref.run(_weights(), toks, key_mask, N_LAYER, N_HEAD, PAD, labels, torch.float64)
    return exact, rounded


def _dev_from(got, exact):
    return float((got.detach().cpu().double() - exact).abs().max()) / float(exact.abs().max())


def test_model_deviates_from_the_exact_model_as_the_rounding_restatement_does(dev):
    from vidsitu_amd.hf_gpt2_fseq import lm_loss

    (lg64, ls64, g64), (lgr, lsr, gr) = _refs()
    toks, labels = _batch()
    m = _model(dev, matmul="bf16").train()
    logits = _train_pass(m, toks.to(dev))
    losses = [lm_loss(logits if i == 0 else logits.detach(), lb.to(dev), PAD) for i, lb in enumerate(labels)]
    losses[0].backward()
    rows = [("logits", logits, lg64, lgr), ("loss", torch.stack([x.detach() for x in losses]), ls64, lsr)]
    rows += [(f"grad {k}", m.P(k).grad, g64[k], gr[k]) for k in g64]
    figures = []
    for name, got, exact, rounded in rows:
        assert bool(torch.isfinite(got).all()), name
        d_ref, d = _dev_from(rounded, exact), _dev_from(got, exact)
        print(f"PARITY gpt2 bf16 [end to end] {name} d_ref={d_ref:.3e} dev={d:.3e} ratio={d / d_ref:.3f}")
        figures.append((name, d_ref, d))
    for name, d_ref, d in figures:
        assert d <= 2 * d_ref, f"{name}: deviation {d:.3e} from the exact model, the restatement's is {d_ref:.3e}"
    name, d_ref, d = figures[0]
    assert d >= d_ref / 2, f"logits deviate by {d:.3e} only (restatement {d_ref:.3e}): is the mode on?"


# ---------------------------------------------------------------------------------------------
# the default is what it was; the decode step is fp32 in both modes
# ---------------------------------------------------------------------------------------------
def test_matmul_fp32_is_the_model_without_the_argument(dev):
    """Bit for bit; the embedding backward adds rows with fp32 atomics whose order is not fixed where several tokens
    meet in one row of dwte / dwpe, so those two are compared bit for bit on a one-row batch of distinct tokens and to
    summation-order noise on the three-row batch (as tests/test_gpu_gpt2_dropout.py does)."""
    old, new, on = _model(dev).train(), _model(dev, matmul="fp32").train(), _model(dev, matmul="bf16").train()
    toks, _ = _batch()
    one_row = torch.randperm(PAD, generator=_gen(5))[:L].view(1, L)
    for t in (toks, one_row):
        td = t.to(dev)
        lo, _, go = _grads_after(old, td)
        ln, _, gn = _grads_after(new, td)
        assert torch.equal(_bits(lo), _bits(ln))
        for k in go:
            if k in ("transformer.wte.weight", "transformer.wpe.weight") and t.shape[0] > 1:
                assert float((go[k] - gn[k]).abs().max()) <= 1e-5 * float(go[k].abs().max()), k
            else:
                assert torch.equal(_bits(go[k]), _bits(gn[k])), k
        lb, _, _ = _grads_after(on, td)
        assert not torch.equal(_bits(lo), _bits(lb))
    old.eval(), new.eval()
    td = toks.to(dev)
    assert torch.equal(_bits(old.forward_logits(td, td.ne(PAD))), _bits(new.forward_logits(td, td.ne(PAD))))


def test_decode_step_and_greedy_tokens_are_the_same_in_both_modes(dev):
    from vidsitu_amd.hf_gpt2_fseq import KVCacheState

    plain, on = _model(dev).eval(), _model(dev, matmul="bf16").eval()
    toks, _ = _batch()
    td = toks.to(dev)
    sa, sb = KVCacheState(), KVCacheState()
    for t in range(3):
        col = td[:, t].contiguous()
        assert torch.equal(_bits(plain.forward_step(col, sa, max_len=8)), _bits(on.forward_step(col, sb, max_len=8)))
    # 17..64 rows: the packed decode step
    wide = torch.randint(0, PAD, (20,), generator=_gen(3)).to(dev)
    sa, sb = KVCacheState(), KVCacheState()
    assert torch.equal(_bits(plain.forward_step(wide, sa, max_len=8)), _bits(on.forward_step(wide, sb, max_len=8)))
    first = td[:, :1].contiguous()
    assert torch.equal(plain.generate_greedy(first, 12, PAD, PAD - 1), on.generate_greedy(first, 12, PAD, PAD - 1))
    assert not torch.equal(_bits(plain.forward_logits(td, td.ne(PAD))), _bits(on.forward_logits(td, td.ne(PAD))))


# ---------------------------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------------------------
def test_captured_training_step_replays_the_eager_step_bit_for_bit(dev):
    """forward_train + LM loss + backward of a bf16-mode model, captured after one eager step: three replays give the
    eager step's loss and gradients bit for bit (split-K slabs are reduced in slice order).  One row of distinct
    tokens, so that the embedding backward's atomics meet nowhere."""
    from vidsitu_amd.hf_gpt2_fseq import lm_loss

    m = _model(dev, matmul="bf16").train()
    td = torch.randperm(PAD, generator=_gen(5))[:L].view(1, L).to(dev)
    _, loss_e, grads_e = _grads_after(m, td)
    m.forward_train(td, td.ne(PAD))  # the backward dropped the transposed weight copies: they exist again from here
    m.take_train_state()
    held = [dict(getattr(m, c)) for c in m._CACHES]  # the captured launches read these copies: they outlive the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = lm_loss(_train_pass(m, td), td, PAD)
        loss.backward()
    for k in range(3):
        for p in m.parameters():
            p.grad.fill_(float("nan"))
        loss.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        print(f"PARITY gpt2 bf16 [graph replay {k}] loss eager={float(loss_e):.9g} replay={float(loss.detach()):.9g}")
        assert torch.equal(_bits(loss.detach().reshape(1)), _bits(loss_e.reshape(1))), f"replay {k}"
        for name in grads_e:
            assert torch.equal(_bits(m.P(name).grad), _bits(grads_e[name])), f"replay {k}: {name}"
    assert held


# ---------------------------------------------------------------------------------------------
# plugin surface
# ---------------------------------------------------------------------------------------------
def test_plugin_surface_tx_only_with_gpt2_matmul_bf16(dev, monkeypatch):
    from vidsitu_amd import ops, synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval
    from vidsitu_amd.optim import ArenaAdam, ParamArena

    cfg = get_cfg({"task_type": "vb_arg", "mdl.mdl_name": "tx_only", "mdl.tx_dec_type": "gpt2",
                   "mdl.gpt2_mdl_name": "gpt2-synth-tiny", "synth.gpt2_vocab": 97, "mdl.gpt2_matmul": "bf16"})
    comm = synth_data.make_comm(cfg)
    sel = get_mdl_loss_eval(cfg)
    torch.manual_seed(0)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev).train()
    gpt2 = [x for x in mdl.modules() if isinstance(x, GPT2LMHeadModelHip)]
    assert len(gpt2) == 1 and gpt2[0].matmul == "bf16"
    loss_fn = sel["loss"](cfg, comm)
    batch = synth_data.synth_srl_batch(comm, bs=2, n_ev=5, seq_len=12, device=dev)
    seen, real = [], ops.gemm_nt
    monkeypatch.setattr(ops, "gemm_nt", lambda *a, **kw: (seen.append(kw.get("bf16", False)), real(*a, **kw))[1])
    loss_fn(mdl(batch), batch)["loss"].backward()
    assert len(seen) >= GEMMS_FWD + GEMMS_BWD and all(seen)
    monkeypatch.setattr(ops, "gemm_nt", real)
    mdl.eval()
    with torch.no_grad():
        before = float(loss_fn(mdl(batch), batch)["loss"])
    mdl.train()
    arena = ParamArena(mdl, adopt_conv=False)
    opt = ArenaAdam(arena, lr=3e-3)
    for _ in range(6):
        opt.zero_grad()
        loss_fn(mdl(batch), batch)["loss"].backward()
        opt.step()
    mdl.eval()
    with torch.no_grad():
        after = float(loss_fn(mdl(batch), batch)["loss"])
    print(f"tx_only with gpt2_matmul = bf16: eval loss {before:.4f} -> {after:.4f} after six Adam steps")
    assert np.isfinite(after) and after < before
    assert arena.data.dtype == torch.float32  # fp32 master weights


def test_main_dist_trains_the_tiny_gpt2_row_with_bf16_matmuls(dev, tmp_path):
    """`python main_dist.py <uid> ... --mdl.gpt2_matmul=bf16` in a fresh child process, as a user's run is: one
    overfitted batch, the loss goes down."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "main_dist.py", "t_gpt2_bf16", "--task_type=vb_arg", "--mdl.mdl_name=tx_only",
           "--mdl.tx_dec_type=gpt2", "--mdl.gpt2_mdl_name=gpt2-synth-tiny", "--synth.gpt2_vocab=97",
           "--mdl.gpt2_matmul=bf16", "--train.bs=2", "--ds.vsitu.num_ev=2", "--train.lr=1e-3", "--overfit_batch=True",
           "--gen.beam_size=2", "--gen.max_len_b=8", f"--misc.tmp_path={tmp_path}", "--steps=4"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    err = "\n".join(ln for ln in r.stderr.splitlines() if "frame #" not in ln)[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + err
    m = re.search(r"loss ([-\d.e]+) -> ([-\d.e]+)", r.stdout)
    assert m, r.stdout
    first, last = float(m.group(1)), float(m.group(2))
    print(f"main_dist tx_only gpt2 bf16: loss {first:.4f} -> {last:.4f}")
    assert "(eager" in r.stdout and np.isfinite(last) and last < first, r.stdout
