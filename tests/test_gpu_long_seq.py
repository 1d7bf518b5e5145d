"""Sequences past the LDS budget of the resident attention kernels, through the models: vidsitu_amd/ops.py hands the
launches the resident kernels refuse to the key-tiled family (csrc/attn_tiled.hip), so RobertaModelHip and
GPT2LMHeadModelHip run up to their position tables.  Before the tiled family these tests raised VsError ("sequence too
long for the LDS-resident attention").

One-layer, one-head modules 64 wide (dh = 64, the head width of roberta-base and gpt2), R = 2, L at the first length the
resident forward refuses -- found with vs_attn_resident_fits -- and for RoBERTa also at a length the resident forward
holds and the resident backward does not (the forward of one family then meets the backward of the other, under
dropout with the same mask).  References: tests/roberta_ref.py / tests/roberta_dropout_ref.py and
tests/gpt2_dropout_ref.py in fp64.  Bounds: RoBERTa as the module-level tests of tests/test_gpu_evrel.py (OUT_TOL,
LOSS_TOL, GRAD_TOL and its _check_grads); GPT-2 as the module-level tests of tests/test_gpu_gpt2_dropout.py
(min(16 * e32, 2e-4) on logits and losses, min(16 * e32, 5e-4) on gradients).  Every figure is printed before it is
asserted.
"""
import functools

import pytest
import torch

import gpt2_dropout_ref as gref
import roberta_dropout_ref as dref
import roberta_ref as ref
from oracle import gpt2_ref
from test_gpu_evrel import LOSS_TOL, OUT_TOL, _check_grads, _rel
from test_gpu_gpt2_dropout import FACTOR, GRAD_CEILING
from test_gpu_gpt2_ops import _check, _errs, _gen

pytestmark = pytest.mark.gpu

SEED = (0x51ed << 32) | 0x2705a3c9
N_LOSSES = 8


def _first_refused(causal, dh, backward):
    from vidsitu_amd import _lib

    lib = _lib.load()
    l = 1
    while lib.vs_attn_resident_fits(causal, l, dh, backward):
        l += 1
    return l


# ---------------------------------------------------------------------------------------------
# RoBERTa
# ---------------------------------------------------------------------------------------------
ROB = dict(n_layer=1, d_model=64, n_head=1, n_positions=200, vocab_size=101, d_ffn=128, pad_token_id=1,
           layer_norm_eps=1e-5)
ROB_R, ROB_STEP = 2, 6


@functools.lru_cache(maxsize=None)
def _rob_batch(l):
    toks, mask = ref.golden_inputs(ROB, ROB_R, l, 13)  # right padding: row 0 full, row 1 three tokens long
    g = _gen(77 + l)
    wh = torch.randn(N_LOSSES, ROB_R, l, ROB["d_model"], generator=g) / (l * ROB["d_model"])
    wp = torch.randn(N_LOSSES, ROB_R, ROB["d_model"], generator=g) / ROB["d_model"]
    return toks, mask, wh, wp


@functools.lru_cache(maxsize=None)
def _rob_ref(l, p_att):
    """fp64: (hidden, pooled), the N_LOSSES losses, the gradients of the first."""
    toks, mask, wh, wp = _rob_batch(l)
    w = {k: v.detach().clone().double().requires_grad_(True) for k, v in ref.make_weights(ROB, 31).items()}
    if p_att:
        h = dref.encoder(w, toks, mask, ROB, dref.masks(SEED, ROB_STEP, ROB, ROB_R, l, 0.0, p_att))
    else:
        h = ref.encoder(w, toks, mask, ROB)
    pooled = ref.pooler(w, h)
    losses = [(h * wh[i].double()).sum() + (pooled * wp[i].double()).sum() for i in range(N_LOSSES)]
    losses[0].backward()
    grads = {k: v.grad for k, v in w.items()}
    for k in grads:  # nn.Embedding(padding_idx = pad): that row of both tables never receives a gradient
        if "word_embeddings" in k or "position_embeddings" in k:
            grads[k][ROB["pad_token_id"]] = 0
    return h.detach(), pooled.detach(), torch.stack([x.detach() for x in losses]), grads


def _rob_run(name, l, p_att, dev):
    from vidsitu_amd import hf_roberta

    toks, mask, wh, wp = _rob_batch(l)
    m = hf_roberta.RobertaModelHip(**ROB, attention_probs_dropout_prob=p_att)
    m.load_state_dict({k: v.float() for k, v in ref.make_weights(ROB, 31).items()}, strict=True)
    m = m.to(dev).train()
    if p_att:
        m.set_dropout_state((SEED, ROB_STEP))
    hidden, pooled = hf_roberta.roberta_apply(m, toks.to(dev), mask.to(dev))
    h64, p64, ls64, g64 = _rob_ref(l, p_att)
    e = (_rel(hidden.view(h64.shape), h64), _rel(pooled, p64))
    print(f"PARITY {name}: hidden {e[0]:.3e} pooler {e[1]:.3e}")
    assert max(e) < OUT_TOL
    losses = [((hidden if i == 0 else hidden.detach()).view(h64.shape) * wh[i].to(dev)).sum()
              + ((pooled if i == 0 else pooled.detach()) * wp[i].to(dev)).sum() for i in range(N_LOSSES)]
    for i, (a, b) in enumerate(zip(losses, ls64)):
        print(f"PARITY {name}: loss {i} {float(a.detach()):.6f} vs {float(b):.6f}")
        assert abs(float(a.detach()) - float(b)) < LOSS_TOL * max(1.0, abs(float(b)))
    losses[0].backward()
    _check_grads({k: m.P(k).grad for k in g64}, g64, name)


@pytest.mark.parametrize("p_att", [0.0, 0.1])
def test_roberta_past_the_resident_forward(p_att, dev):
    """L = 193 at dh = 64: the tiled forward and the tiled backward."""
    l = _first_refused(0, 64, 0)
    assert l == 193
    _rob_run(f"roberta long L{l} p_att={p_att}", l, p_att, dev)


@pytest.mark.parametrize("p_att", [0.0, 0.1])
def test_roberta_resident_forward_tiled_backward(p_att, dev):
    """145 <= L <= 192: the resident forward still holds the sequence, the resident backward does not."""
    from vidsitu_amd import _lib

    l = 160
    lib = _lib.load()
    assert lib.vs_attn_resident_fits(0, l, 64, 0) == 1 and lib.vs_attn_resident_fits(0, l, 64, 1) == 0
    _rob_run(f"roberta mixed L{l} p_att={p_att}", l, p_att, dev)


# ---------------------------------------------------------------------------------------------
# GPT-2
# ---------------------------------------------------------------------------------------------
G_LAYER, G_D, G_HEAD, G_POS, G_VOCAB = 1, 64, 1, 320, 97
G_PAD = G_VOCAB - 1
G_R, G_NPAD, G_STEP = 2, 7, 6


@functools.lru_cache(maxsize=None)
def _g_weights():
    return {k: torch.from_numpy(v) for k, v in gpt2_ref.make_weights(G_VOCAB, G_POS, G_D, G_LAYER, 23).items()}


@functools.lru_cache(maxsize=None)
def _g_batch(l):
    """Row 1 is left-padded.  The queries in front of the padding see no unmasked key; as in training they carry no
    loss: position G_NPAD - 1 would predict the row's first token, which every label set therefore ignores."""
    g = _gen(79 + l)
    toks = torch.randint(0, G_PAD, (G_R, l), generator=g)
    toks[1, :G_NPAD] = G_PAD
    labels = [toks] + [torch.where(toks == G_PAD, toks, torch.randint(0, G_PAD, (G_R, l), generator=g))
                       for _ in range(N_LOSSES - 1)]
    labels = [lb.clone() for lb in labels]
    for lb in labels:
        lb[1, G_NPAD] = G_PAD
    return toks, labels


@functools.lru_cache(maxsize=None)
def _g_ref(l, p_attn):
    toks, labels = _g_batch(l)
    drops = gref.masks(SEED, G_STEP, G_LAYER, G_R, l, G_D, G_HEAD, 0.0, p_attn, 0.0)
    return [gref.run(_g_weights(), toks, toks.ne(G_PAD), G_LAYER, G_HEAD, drops, G_PAD, labels, dt)
            for dt in (torch.float64, torch.float32)]


def _g_model(dev, **pdrop):
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip

    m = GPT2LMHeadModelHip(G_LAYER, G_D, G_HEAD, G_POS, G_VOCAB, **pdrop)
    sd = dict(_g_weights())
    sd["lm_head.weight"] = sd["transformer.wte.weight"]
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def _visible(l):
    """[R, L] bool: the positions whose query has an unmasked visible key (all but the left padding of row 1)."""
    v = torch.ones(G_R, l, dtype=torch.bool)
    v[1, :G_NPAD] = False
    return v


@pytest.mark.parametrize("p_attn", [0.0, 0.1])
def test_gpt2_past_the_resident_forward(p_attn, dev):
    """L = 304: forward_train + loss + backward (and forward_logits at p = 0) through the tiled kernels, one row
    left-padded.  The logits at the left padding itself are good to FULLY_MASKED_BOUND only
    (tests/test_gpu_gpt2_ops.py) and feed no loss: they are left out of the logits comparison."""
    from vidsitu_amd.hf_gpt2_fseq import _GPT2TrainFn, lm_loss

    l = _first_refused(1, 64, 0)
    assert l == 304 and l <= G_POS
    name = f"gpt2 long L{l} attn_pdrop={p_attn}"
    toks, labels = _g_batch(l)
    (lg64, ls64, g64), (lg32, ls32, g32) = _g_ref(l, p_attn)
    vis = _visible(l)
    toks_d = toks.to(dev)
    if p_attn == 0.0:
        lg = _g_model(dev).eval().forward_logits(toks_d, toks_d.ne(G_PAD))
        _check(f"{name} forward_logits", lg[vis.to(dev)], lg64[vis], lg32[vis])
    m = _g_model(dev, attn_pdrop=p_attn).train()
    if p_attn:
        m.set_dropout_state((SEED, G_STEP))
    tick = torch.zeros(1, device=dev, requires_grad=True)
    logits = _GPT2TrainFn.apply(m, toks_d, toks_d.ne(G_PAD), tick)
    assert bool(torch.isfinite(logits).all())
    _check(f"{name} logits", logits.detach()[vis.to(dev)], lg64[vis], lg32[vis])
    losses = [lm_loss(logits if i == 0 else logits.detach(), lb.to(dev), G_PAD) for i, lb in enumerate(labels)]
    _check(f"{name} loss", torch.stack([x.detach() for x in losses]), ls64, ls32)
    losses[0].backward()
    for k in g64:
        got = m.P(k).grad
        assert bool(torch.isfinite(got).all()), f"{name} {k}: non-finite gradient"
        e32, err = _errs(got, g64[k], g32[k])
        print(f"PARITY {name} grad {k} e32={e32:.3e} err={err:.3e}")
        assert err <= min(FACTOR * e32, GRAD_CEILING), f"{name} grad {k}: {err:.3e} vs fp32 floor {e32:.3e}"


def test_generate_greedy_from_a_long_prompt(dev):
    """A prompt past the resident forward limit: generate_greedy (the cached decode step, vs_attn_decode, position by
    position) returns the tokens of a loop of forward_logits argmaxes (the whole sequence through the tiled kernel
    every time) on the same module.  No row emits the end token here (it is outside the vocabulary)."""
    plen, n_new = _first_refused(1, 64, 0) + 1, 6
    assert plen + n_new <= G_POS
    m = _g_model(dev).eval()
    prompt = torch.randint(0, G_PAD, (G_R, plen), generator=_gen(5)).to(dev)
    got = m.generate_greedy(prompt, plen + n_new, G_PAD, G_VOCAB)
    seq = prompt
    for _ in range(n_new):
        lg = m.forward_logits(seq)[:, -1]
        top2 = lg.topk(2, dim=-1).values
        print(f"generate_greedy L{seq.shape[1]}: smallest top-2 logit gap {float((top2[:, 0] - top2[:, 1]).min()):.3e}")
        seq = torch.cat([seq, lg.argmax(-1, keepdim=True)], dim=1)
    assert tuple(got.shape) == (G_R, plen + n_new)
    assert torch.equal(got, seq)


# ---------------------------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True], ids=["pad", "causal"])
def test_tiled_launches_are_capturable(causal, dev):
    """After one eager call (the LDS attribute of the kernels, the workspace) forward and backward are captured in a
    graph like their resident siblings; the replay gives the eager bits."""
    from vidsitu_amd import ops

    r, l, h, dh = 2, 320, 2, 64
    assert ops._lib.load().vs_attn_resident_fits(int(causal), l, dh, 0) == 0
    g = _gen(3)
    qkv = torch.randn(r * l, 3 * h * dh, generator=g).to(dev)
    dout = torch.randn(r * l, h * dh, generator=g).to(dev)
    mask = torch.ones(r, l, dtype=torch.uint8)
    mask[1, l - 9:] = 0
    mask = mask.to(dev)
    drop = (torch.tensor([SEED, 4], dtype=torch.int64, device=dev), 1) + ops.dropout_params(0.1)
    fwd, bwd = (ops.attn_causal, ops.attn_causal_bwd) if causal else (ops.attn_pad, ops.attn_pad_bwd)
    eager = (fwd(qkv, mask, r, l, h, drop=drop), bwd(qkv, mask, dout, r, l, h, drop=drop))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fwd(qkv, mask, r, l, h, drop=drop)
        dqkv = bwd(qkv, mask, dout, r, l, h, drop=drop)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0]) and torch.equal(dqkv, eager[1])
