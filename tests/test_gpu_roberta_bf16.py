"""`_RobertaHip(..., matmul="bf16")` (`mdl.rob_matmul`): bf16 operands with fp32 accumulation in the encoder's dense
layers -- the fused q/k/v projection, attention.output.dense, intermediate.dense, output.dense -- forward and backward,
the backward through the K-strided forms of `ops.gemm_bf16` (no transposed copy), fp32 everywhere else, the default
untouched.

roberta_ref.TINY with `roberta_ref.make_weights(TINY, 31)`; R = 3, L = 23, one right-padded row: 69 tokens, so the dW
products have K = 69 (no multiple of 4, nor of 2).  roberta_ref.WIDE (d = 768, ffn = 3072) at R = 2, L = 40 runs the
split-K and 64-tile branches inside the model.

Every call, tightly: `ops.gemm_nt`, `ops.gemm_bf16` and `ops.transpose_f32` are wrapped for one bf16-mode forward_train
+ backward and one eval forward; every encoder dense call's own recorded operands go through the restatement of
tests/test_gpu_gemm_bf16.py (operands rounded with `tensor.bfloat16()`, fp64; `e32` = the same in fp32) under the rule
err <= min(16 * e32, 2e-4).  As tests/test_gpu_gpt2_bf16.py explains, this is the tight whole-model check: an end
result cannot be held tightly to a restatement that rounds at every GEMM, because an activation that lands on the other
side of a bf16 rounding boundary moves the result by far more than fp32 noise.

End to end, loosely (that file's rule): `d_ref` = the fp64 deviation of tests/roberta_bf16_ref.py (dense layers that
round x, W and dy to bf16) from the exact fp64 model, relative to max |exact|.  The model's deviation from the exact
model must be at most 2 * d_ref for the last hidden state, the logits, the loss vector and every parameter gradient,
and at least d_ref / 2 for the last hidden state (the mode is really on).  `attention.self.key.bias` has an
analytically zero gradient -- exact model, restatement and kernel all hold rounding noise only -- so it is held, as
tests/test_gpu_roberta_dropout.py holds it, to min(16 * e32, 2e-4) on the scale of the model's largest gradient entry,
e32 = the restatement's own fp32 noise.  Every figure is printed (`PARITY ...`) before it is asserted."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import roberta_bf16_ref as bref
import roberta_ref as ref
from test_gpu_gemm_bf16 import ACT_NAMES, _restate
from test_gpu_gpt2_ops import CEILING, FACTOR, _bits, _errs, _gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (0x51ed << 32) | 0x2705a3c9
N_LOSSES = 8
# L = 193 is the first length the resident forward refuses at roberta-base's head width of 64 (TINY's two heads are 32
# wide, which the resident kernels hold up to a longer L): one head of 64 over TINY's d_model
LONG = dict(ref.TINY, n_positions=200, n_head=1)
CASES = {"tiny": (ref.TINY, 3, 23), "wide": (ref.WIDE, 2, 40), "long": (LONG, 1, 193)}


@functools.lru_cache(maxsize=None)
def _batch(case):
    """Right-padded tokens: row 1 (when there is one) five tokens short, the others full."""
    dims, r, l = CASES[case]
    g = _gen(77 + l)
    toks = torch.randint(4, dims["vocab_size"], (r, l), generator=g)
    mask = torch.ones((r, l), dtype=torch.long)
    toks[:, 0] = 0
    if r > 1:
        toks[1, l - 5:] = dims["pad_token_id"]
        mask[1, l - 5:] = 0
    for i in range(r):
        toks[i, int(mask[i].sum()) - 1] = 2
    labels = torch.randint(0, 5, (N_LOSSES, r), generator=g)
    wh = torch.randn(r, l, dims["d_model"], generator=g) / (l * dims["d_model"])
    return toks, mask, labels, wh


@functools.lru_cache(maxsize=None)
def _weights(case, kind):
    dims = CASES[case][0]
    if kind == "cls":
        return ref.make_weights(dims, 31, prefix="roberta.", pooler=False, num_labels=5)
    return ref.make_weights(dims, 31)


def _model(case, kind, dev, **kw):
    from vidsitu_amd.hf_roberta import RobertaForSequenceClassificationHip, RobertaModelHip

    dims = CASES[case][0]
    m = RobertaForSequenceClassificationHip(**dims, num_labels=5, **kw) if kind == "cls" else RobertaModelHip(**dims, **kw)
    m.load_state_dict({k: v.float() for k, v in _weights(case, kind).items()}, strict=True)
    return m.to(dev)


def _apply(m, case, dev):
    from vidsitu_amd import hf_roberta

    toks, mask, *_ = _batch(case)
    return hf_roberta.roberta_apply(m, toks.to(dev), mask.to(dev))


def _hidden_loss(case, hidden):
    return (hidden * _batch(case)[3].to(hidden.device)).sum()


# ---------------------------------------------------------------------------------------------
# every GEMM call of the mode, each against the restatement from its own operands
# ---------------------------------------------------------------------------------------------
def _cpu(t):
    return None if t is None else t.detach().cpu().clone()


def _recording(monkeypatch):
    """Wraps ops.gemm_nt, ops.gemm_bf16 and ops.transpose_f32.  A record holds the LOGICAL operands A [M, K], B [N, K]."""
    from vidsitu_amd import ops

    calls, real_nt, real_bf, real_tr = [], ops.gemm_nt, ops.gemm_bf16, ops.transpose_f32

    def gemm_nt(x, w, b=None, res=None, act=ops.ACT_NONE, out=None, bf16=False):
        rec = dict(op="gemm_nt", x=_cpu(x), w=_cpu(w), b=_cpu(b), res=_cpu(res), act=int(act), bf16=bf16, forms=(0, 0))
        y = real_nt(x, w, b, res, act=act, out=out, bf16=bf16)
        rec["y"] = _cpu(y)
        calls.append(rec)
        return y

    def gemm_bf16(a, b, bias=None, res=None, act=ops.ACT_NONE, out=None, a_t=False, b_t=False):
        rec = dict(op="gemm_bf16", x=_cpu(a.t() if a_t else a).contiguous(), w=_cpu(b.t() if b_t else b).contiguous(),
                   b=_cpu(bias), res=_cpu(res), act=int(act), bf16=True, forms=(int(a_t), int(b_t)))
        y = real_bf(a, b, bias, res, act=act, out=out, a_t=a_t, b_t=b_t)
        rec["y"] = _cpu(y)
        calls.append(rec)
        return y

    def transpose_f32(x):
        calls.append(dict(op="transpose_f32", shape=tuple(x.shape)))
        return real_tr(x)

    monkeypatch.setattr(ops, "gemm_nt", gemm_nt)
    monkeypatch.setattr(ops, "gemm_bf16", gemm_bf16)
    monkeypatch.setattr(ops, "transpose_f32", transpose_f32)
    return calls


def _check_calls(name, calls):
    for i, c in enumerate(calls):
        assert c["bf16"] is True, f"{name}: call {i} ran with fp32 operands"
        (m, k), n = c["x"].shape, c["w"].shape[0]
        ref64 = _restate(c["x"], c["w"], c["b"], c["res"], c["act"], torch.float64)
        ref32 = _restate(c["x"], c["w"], c["b"], c["res"], c["act"], torch.float32)
        e32, err = _errs(c["y"], ref64, ref32)
        tag = (f"{name} call {i} {c['op']} forms={c['forms']} M={m} N={n} K={k} act={ACT_NAMES[c['act']]}"
               + (" bias" if c["b"] is not None else ""))
        print(f"PARITY {tag} e32={e32:.3e} err={err:.3e}")
        assert bool(torch.isfinite(c["y"]).all()), tag
        assert err <= min(FACTOR * e32, CEILING), f"{tag}: kernel error {err:.3e} vs fp32 floor {e32:.3e}"


def _encoder_calls(calls, case):
    """The GEMM records of the encoder's dense layers; what is left must be the pooler's fp32 GEMM on R rows."""
    _, r, l = CASES[case]
    gemms = [c for c in calls if c["op"] != "transpose_f32"]
    head = [c for c in gemms if c["op"] == "gemm_nt" and c["x"].shape[0] == r]
    assert all(c["bf16"] is False for c in head), "the pooler stays fp32"
    return [c for c in gemms if not any(c is h for h in head)]


def _train_and_eval_calls(case, dev, monkeypatch, **kw):
    """One forward_train + backward (loss on the last hidden state) and one eval forward of a bf16-mode RobertaModelHip
    under the recorder -> (forward calls, backward calls, eval calls), counts asserted."""
    dims, r, l = CASES[case]
    n = dims["n_layer"]
    m = _model(case, "pool", dev, matmul="bf16", **kw).train()
    if kw:
        m.set_dropout_state((SEED, 5))
    calls = _recording(monkeypatch)
    hidden, _ = _apply(m, case, dev)
    fwd = _encoder_calls(calls, case)
    n_fwd_all = len(calls)
    assert len(fwd) == 4 * n and all(c["op"] == "gemm_nt" for c in fwd)
    _hidden_loss(case, hidden).backward()
    torch.cuda.synchronize()
    back = calls[n_fwd_all:]
    assert [c for c in back if c["op"] == "transpose_f32"] == [], "the bf16 backward makes no transposed copy"
    assert all(c["op"] == "gemm_bf16" for c in back)
    assert len(back) == (6 + 4) * n, "dW and dx of three layers, three dW and one dx of the fused projection"
    forms = sorted({c["forms"] for c in back})
    assert forms == [(0, 1), (1, 1)], "dx: B strided; dW: both strided"
    assert r * l in {c["x"].shape[1] for c in back if c["forms"] == (1, 1)}, "the dW GEMMs sum over the tokens"
    del calls[:]
    m.eval()
    toks, mask, *_ = _batch(case)
    m(toks.to(dev), mask.to(dev))
    ev = _encoder_calls(calls, case)
    assert len(ev) == 4 * n and not [c for c in calls if c["op"] == "transpose_f32"]
    # the cached transposed q/k/v weight is not built in this mode
    assert all(t[2] is None for t in m._qkv.values()) and len(m._qkv) == n
    return fwd, back, ev


@pytest.mark.parametrize("case", ["tiny", "wide"])
def test_every_encoder_gemm_takes_bf16_operands_and_matches_its_restatement(case, dev, monkeypatch):
    fwd, back, ev = _train_and_eval_calls(case, dev, monkeypatch)
    if case == "tiny":
        assert (3 * 23) % 2 == 1  # K = 69: the last k-pair of the dW products is half outside
    _check_calls(f"roberta bf16 {case} forward_train", fwd)
    _check_calls(f"roberta bf16 {case} backward", back)
    _check_calls(f"roberta bf16 {case} eval forward", ev)


def test_wide_case_runs_the_split_k_and_64_tile_branches(dev):
    from vidsitu_amd import ops

    lib = ops._lib.load()
    t, d, f = 80, 768, 3072
    assert lib.vs_gemm_nt_bf16_workspace_bytes(t, f, d) > 0 and lib.vs_gemm_nt_bf16_workspace_bytes(t, d, f) > 0  # split-K
    assert lib.vs_gemm_nt_bf16_workspace_bytes(f, d, t) == 0  # the dW products: unsplit 64 x 64 tiles


def test_long_sequence_runs_on_the_key_tiled_attention(dev, monkeypatch):
    """L = 193, the first length the resident forward refuses (head width 64)."""
    from vidsitu_amd import ops

    lib = ops._lib.load()
    dh = LONG["d_model"] // LONG["n_head"]
    assert lib.vs_attn_resident_fits(0, 192, dh, 0) == 1 and lib.vs_attn_resident_fits(0, 193, dh, 0) == 0
    fwd, back, ev = _train_and_eval_calls("long", dev, monkeypatch)
    _check_calls("roberta bf16 L=193 forward_train", fwd)
    _check_calls("roberta bf16 L=193 backward", back)


# ---------------------------------------------------------------------------------------------
# end to end against the rounding restatement
# ---------------------------------------------------------------------------------------------
def _ref_run(enc, dtype, **kw):
    """(hidden of the pooled model's weights, logits, losses, grads of the first loss) of the classification model."""
    dims = ref.TINY
    toks, mask, labels, _ = _batch("tiny")
    w = {k: v.to(dtype).clone().requires_grad_(True) for k, v in _weights("tiny", "cls").items()}
    h = enc(w, toks, mask, dims, prefix="roberta.", **kw)
    logits = ref.classifier(w, h)
    losses = torch.stack([torch.nn.functional.cross_entropy(logits, lb) for lb in labels])
    names = list(w)
    grads = dict(zip(names, torch.autograd.grad(losses[0], [w[k] for k in names])))
    for k in grads:  # nn.Embedding(padding_idx = pad): that row of both tables never receives a gradient
        if "word_embeddings" in k or "position_embeddings" in k:
            grads[k][dims["pad_token_id"]] = 0
    return h.detach(), logits.detach(), losses.detach(), grads


@functools.lru_cache(maxsize=None)
def _refs():
    return (_ref_run(ref.encoder, torch.float64), _ref_run(bref.encoder, torch.float64),
            _ref_run(bref.encoder, torch.float32))


def _dev_from(got, exact, top=None):
    return float((got.detach().cpu().double() - exact).abs().max()) / (top or float(exact.abs().max()))


def test_model_deviates_from_the_exact_model_as_the_rounding_restatement_does(dev):
    from vidsitu_amd.mdl_sf_base import hip_cross_entropy

    (h64, lg64, ls64, g64), (hr, lgr, lsr, gr), (_, _, _, gr32) = _refs()
    toks, mask, labels, _ = _batch("tiny")
    # the same encoder weights under both prefixes (make_weights draws the encoder first)
    pool, cls = _weights("tiny", "pool"), _weights("tiny", "cls")
    assert all(torch.equal(pool[k], cls["roberta." + k]) for k in pool if not k.startswith("pooler."))
    hidden = _model("tiny", "pool", dev, matmul="bf16").eval()(toks.to(dev), mask.to(dev)).last_hidden_state
    m = _model("tiny", "cls", dev, matmul="bf16").train()
    (logits,) = _apply(m, "tiny", dev)
    losses = [hip_cross_entropy(logits if i == 0 else logits.detach(), lb.to(dev)) for i, lb in enumerate(labels)]
    losses[0].backward()
    key_bias = [k for k in g64 if k.endswith("attention.self.key.bias")]
    rows = [("last hidden state", hidden, h64, hr), ("logits", logits, lg64, lgr),
            ("loss", torch.stack([x.detach() for x in losses]), ls64, lsr)]
    rows += [(f"grad {k}", m.P(k).grad, g64[k], gr[k]) for k in g64 if k not in key_bias]
    figures = []
    for name, got, exact, rounded in rows:
        assert got is not None and bool(torch.isfinite(got).all()), name
        d_ref, d = _dev_from(rounded, exact), _dev_from(got, exact)
        print(f"PARITY roberta bf16 [end to end] {name} d_ref={d_ref:.3e} dev={d:.3e} ratio={d / d_ref:.3f}")
        figures.append((name, d_ref, d))
    top = max(float(v.abs().max()) for v in g64.values())
    zeros = []
    for k in key_bias:
        e32, err = _dev_from(gr32[k], gr[k], top), _dev_from(m.P(k).grad, gr[k], top)
        print(f"PARITY roberta bf16 [end to end] grad {k} (analytically zero; on the model's scale {top:.3e}) "
              f"e32={e32:.3e} err={err:.3e}")
        zeros.append((k, e32, err))
    for name, d_ref, d in figures:
        assert d <= 2 * d_ref, f"{name}: deviation {d:.3e} from the exact model, the restatement's is {d_ref:.3e}"
    for k, e32, err in zeros:
        assert err <= min(FACTOR * e32, CEILING), f"{k}: {err:.3e} vs fp32 floor {e32:.3e}"
    name, d_ref, d = figures[0]
    assert d >= d_ref / 2, f"the hidden state deviates by {d:.3e} only (restatement {d_ref:.3e}): is the mode on?"


# ---------------------------------------------------------------------------------------------
# the default is what it was
# ---------------------------------------------------------------------------------------------
def _grads_after(m, case, kind, dev):
    from vidsitu_amd import _lib
    from vidsitu_amd.mdl_sf_base import hip_cross_entropy

    for p in m.parameters():
        p.grad = None
    before = _lib.load().vs_launch_count()
    outs = _apply(m, case, dev)
    if kind == "cls":
        hip_cross_entropy(outs[0], _batch(case)[2][0].to(dev)).backward()
    else:
        (_hidden_loss(case, outs[0]) + outs[1].sum()).backward()
    torch.cuda.synchronize()
    return ([o.detach().clone() for o in outs], {k: m.P(k).grad.clone() for k in m._names},
            _lib.load().vs_launch_count() - before)


def _same_grads(ga, gb):
    for k in ga:  # the two embedding tables' backward adds rows with fp32 atomics: summation-order noise
        if "word_embeddings" in k or "position_embeddings" in k:
            assert float((ga[k] - gb[k]).abs().max()) <= 1e-5 * float(ga[k].abs().max()), k
        else:
            assert torch.equal(_bits(ga[k]), _bits(gb[k])), k


@pytest.mark.parametrize("kind", ["pool", "cls"])
def test_matmul_fp32_is_the_model_without_the_argument(kind, dev, monkeypatch):
    from vidsitu_amd import ops

    old, new = _model("tiny", kind, dev).train(), _model("tiny", kind, dev, matmul="fp32").train()
    on = _model("tiny", kind, dev, matmul="bf16").train()
    seen, real = [], ops.gemm_bf16
    monkeypatch.setattr(ops, "gemm_bf16", lambda *a, **kw: (seen.append(1), real(*a, **kw))[1])
    for m in (old, new):  # the fused q/k/v weights exist on both sides from here on
        _grads_after(m, "tiny", kind, dev)
    oo, go, no = _grads_after(old, "tiny", kind, dev)
    on_, gn, nn_ = _grads_after(new, "tiny", kind, dev)
    print(f"LAUNCHES {kind}: {no} without the argument, {nn_} with matmul='fp32'")
    assert seen == [], "the default model issues no ops.gemm_bf16 call"
    assert no == nn_ and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(oo, on_))
    _same_grads(go, gn)
    ob, _, nb = _grads_after(on, "tiny", kind, dev)
    assert seen and not torch.equal(_bits(oo[0]), _bits(ob[0]))
    print(f"LAUNCHES {kind}: {nb} with matmul='bf16'")
    old.eval(), new.eval()
    toks, mask, *_ = _batch("tiny")
    key = "logits" if kind == "cls" else "last_hidden_state"
    assert torch.equal(_bits(old(toks.to(dev), mask.to(dev))[key]), _bits(new(toks.to(dev), mask.to(dev))[key]))


# ---------------------------------------------------------------------------------------------
# dropout composes
# ---------------------------------------------------------------------------------------------
def test_dropout_composes_with_the_mode(dev, monkeypatch):
    drop = dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    m = _model("tiny", "cls", dev, matmul="bf16", **drop).train()
    plain = _model("tiny", "cls", dev, matmul="bf16").train()
    m.set_dropout_state((SEED, 9))
    o1, g1, _ = _grads_after(m, "tiny", "cls", dev)
    assert m.dropout_state() == (SEED, 10)
    m.set_dropout_state((SEED, 9))
    o2, g2, _ = _grads_after(m, "tiny", "cls", dev)
    assert torch.equal(_bits(o1[0]), _bits(o2[0]))
    _same_grads(g1, g2)
    o3, _, _ = _grads_after(m, "tiny", "cls", dev)  # step 10: other masks
    op, _, _ = _grads_after(plain, "tiny", "cls", dev)
    assert not torch.equal(o1[0], o3[0]) and not torch.equal(o1[0], op[0])
    fwd, back, ev = _train_and_eval_calls("tiny", dev, monkeypatch, **drop)
    _check_calls("roberta bf16 dropout 0.1 forward_train", fwd)
    _check_calls("roberta bf16 dropout 0.1 backward", back)


# ---------------------------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------------------------
def test_captured_training_step_replays_the_eager_step_bit_for_bit(dev):
    """Forward + loss + backward of a bf16-mode model, captured after one eager step: three replays give the eager
    step's loss and gradients bit for bit (split-K slabs are reduced in slice order).  One row of distinct tokens, so
    that the embedding backward's atomics meet nowhere."""
    from vidsitu_amd import hf_roberta
    from vidsitu_amd.mdl_sf_base import hip_cross_entropy

    dims = ref.TINY
    m = _model("tiny", "cls", dev, matmul="bf16").train()
    td = (4 + torch.randperm(dims["vocab_size"] - 4, generator=_gen(5))[:23]).view(1, 23).to(dev)
    md = torch.ones_like(td)
    lab = torch.tensor([3], device=dev)

    def step():
        (logits,) = hf_roberta.roberta_apply(m, td, md)
        loss = hip_cross_entropy(logits, lab)
        loss.backward()
        return loss

    for p in m.parameters():
        p.grad = None
    loss_e = step().detach().clone()
    torch.cuda.synchronize()
    grads_e = {k: m.P(k).grad.clone() for k in m._names}
    m.forward_train(td, md)  # the backward dropped the fused q/k/v copies: they exist again from here
    m.take_train_state()
    held = [dict(getattr(m, c)) for c in m._CACHES]  # the captured launches read these copies: they outlive the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    for k in range(3):
        for p in m.parameters():
            p.grad.fill_(float("nan"))
        loss.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        print(f"PARITY roberta bf16 [graph replay {k}] loss eager={float(loss_e):.9g} replay={float(loss.detach()):.9g}")
        assert torch.equal(_bits(loss.detach().reshape(1)), _bits(loss_e.reshape(1))), f"replay {k}"
        for name in grads_e:
            assert torch.equal(_bits(m.P(name).grad), _bits(grads_e[name])), f"replay {k}: {name}"
    assert held


# ---------------------------------------------------------------------------------------------
# plugin surface
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["rob_evrel", "sfpret_evrel"])
def test_plugin_surface_with_rob_matmul_bf16(row, dev, monkeypatch):
    """One training step through get_mdl_loss_eval at mdl.rob_matmul = bf16: finite loss, finite non-zero gradients on
    the encoder's weights, every encoder GEMM through the bf16 entries."""
    from vidsitu_amd import ops, synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.hf_roberta import _RobertaHip
    from vidsitu_amd.mdl_sf_base import get_head_dim
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    cfg = get_cfg({"task_type": "evrel", "mdl.mdl_name": row, "mdl.rob_mdl_name": "roberta-synth-tiny",
                   "mdl.rob_matmul": "bf16"})
    comm = synth_data.make_comm(cfg)
    sel = get_mdl_loss_eval(cfg)
    torch.manual_seed(0)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev).train()
    (rob,) = [x for x in mdl.modules() if isinstance(x, _RobertaHip)]
    assert rob.matmul == "bf16"
    batch = {k: v.to(dev) for k, v in
             synth_data.synth_evrel_batch(comm, 2, n_ann=1, feat_dim=get_head_dim(cfg), seed=41).items()}
    seen, real = [], ops.gemm_bf16
    monkeypatch.setattr(ops, "gemm_bf16", lambda *a, **kw: (seen.append(1), real(*a, **kw))[1])
    loss = sel["loss"](cfg, comm)(mdl(batch), batch)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    print(f"{row} with rob_matmul = bf16: loss {float(loss.detach()):.6f}, {len(seen)} gemm_bf16 calls")
    assert np.isfinite(float(loss.detach())) and len(seen) == 10 * rob.n_layer
    for i in range(rob.n_layer):
        for leaf in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
                     "intermediate.dense", "output.dense"):
            g = rob.E(f"encoder.layer.{i}.{leaf}.weight").grad
            assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, leaf


def test_main_dist_trains_sfpret_evrel_with_bf16_matmuls(dev, tmp_path):
    """`python main_dist.py <uid> --task_type=evrel ... --mdl.rob_matmul=bf16` in a fresh child process, as a user's
    run is: one overfitted batch, the loss goes down."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    cmd = [sys.executable, "main_dist.py", "t_evrel_bf16", "--task_type=evrel", "--mdl.mdl_name=sfpret_evrel",
           "--mdl.rob_mdl_name=roberta-synth-tiny", "--mdl.rob_matmul=bf16", "--train.bs=2", "--train.lr=1e-3",
           "--overfit_batch=True", f"--misc.tmp_path={tmp_path}", "--steps=3", "--num_gpus=1"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    err = "\n".join(ln for ln in r.stderr.splitlines() if "frame #" not in ln)[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + err
    m = re.search(r"loss ([-\d.e]+) -> ([-\d.e]+)", r.stdout)
    assert m and "(eager" in r.stdout, r.stdout
    first, last = float(m.group(1)), float(m.group(2))
    print(f"main_dist sfpret_evrel rob_matmul=bf16: loss {first:.4f} -> {last:.4f}")
    assert np.isfinite(last) and last < first, r.stdout
