"""Train-mode dropout of the RoBERTa encoder from the in-kernel counter generator (csrc/dropout_rng.h): the attention
kernels' DROP instantiation, the residual site LayerNorm(res + m o b), the two host models, the [seed, step] state and
the evrel plugin surface.

Masks come from the CPU restatement (tests/dropout_ref.py); values are held to the rule of
tests/test_gpu_roberta_ops.py: kernel error <= min(16 * e32, 2e-4) against an fp64 torch restatement with mask
operands (tests/roberta_dropout_ref.py), e32 = the same restatement's fp32 noise floor with the same masks, both
relative to max |fp64|; a quantity whose fp64 value is exactly zero must be exactly zero.  A mask wrong at a single
element moves a value by order 1, so the value tests are the mask tests.  `attention.self.key.bias` has an analytically
zero gradient (the rows of dS sum to zero with dropout too): both sides hold rounding noise, and it is measured on the
scale of the model's largest gradient entry, as tests/test_gpu_evrel.py does.  Every figure is printed (`PARITY ...`)
before it is asserted.
"""
import functools

import pytest
import torch

import dropout_ref
import roberta_dropout_ref as dref
import roberta_ref as ref
from test_gpu_roberta_ops import CEILING, FACTOR, MASKS, _attn_case, _bwd_poisoned, _check, _gen

pytestmark = pytest.mark.gpu

NAN = float("nan")
SEED = (0x51ed << 32) | 0x2705a3c9  # above 2^32: both key words in play


def _bits(t):
    return t.contiguous().view(torch.int32)


def _drop(dev, seed, step, site, p):
    from vidsitu_amd import ops

    return (torch.tensor([seed, step], dtype=torch.int64, device=dev), site) + ops.dropout_params(p)


def _zeros_stay_zero(name, got, ref64):
    """Element by element: where the fp64 value is exactly zero (a query whose keys were all dropped, a key nobody
    kept, a masked key) the kernel's is exactly zero."""
    z = (ref64 == 0).to(got.device)
    assert bool((got[z] == 0).all()), f"{name}: an exactly-zero element is not zero"


# ---------------------------------------------------------------------------------------------
# attention with dropout on the probabilities
# ---------------------------------------------------------------------------------------------
ATTN_STEP, ATTN_SITE = 3, 4
ATTN_P = (0.1, 0.5)


@functools.lru_cache(maxsize=None)
def _attn_drop_case(r, l, h, dh, kind, p):
    """fp64 / fp32 references with the step's mask, on the inputs of the plain case: computed once, left unchanged."""
    c = _attn_case(r, l, h, dh, kind)
    d = h * dh
    thr, scale = dropout_ref.threshold(p)
    keep = torch.from_numpy(dropout_ref.keep_attn(SEED, ATTN_STEP, ATTN_SITE, r, h, l, thr)).double() * scale
    out = {}
    for dt in (torch.float64, torch.float32):
        x = c["qkv"].view(r, l, 3 * d).to(dt).requires_grad_(True)
        o = dref.attention(x, c["mask"], h, keep)
        (gx,) = torch.autograd.grad(o, x, c["dout"].view(r, l, d).to(dt))
        out[dt] = (o.detach().reshape(r * l, d), gx.reshape(r * l, 3 * d))
    return dict(o64=out[torch.float64][0], g64=out[torch.float64][1], o32=out[torch.float32][0],
                g32=out[torch.float32][1])


def _drop_bwd_poisoned(ops, qkv_d, mask_d, dout_d, r, l, h, dh, drop, dev):
    """vs_attn_pad_drop_bwd through the C ABI with dqkv and the whole scratch workspace full of NaN."""
    need = ops._lib.load().vs_attn_pad_bwd_scratch_bytes(r, l, h)
    ws = ops._workspace(need, dev)
    ws.view(torch.float32).fill_(NAN)
    dqkv = torch.full_like(qkv_d, NAN)
    snap, site, thr, scale = drop
    ops._lib.call("vs_attn_pad_drop_bwd", ops._ptr(qkv_d), ops._ptr(mask_d), ops._ptr(dout_d), ops._ptr(dqkv),
                  ops._ptr(ws), ws.numel(), r, l, h, dh, ops._ptr(snap), site, thr, scale, ops._stream())
    return dqkv


@pytest.mark.parametrize("h", [1, 2])
@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("l", [1, 5, 16, 17, 65, 120])
def test_attn_pad_drop_fwd_bwd(l, dh, h, dev):
    """Every mask kind and both probabilities at this shape.  The plain entry points run first and are recorded; after
    the DROP calls they give the same bits (one template) and still meet the fp64 bound."""
    from vidsitu_amd import ops

    r = 3
    d = h * dh
    for kind in MASKS:
        c = _attn_case(r, l, h, dh, kind)
        qkv_d, dout_d = c["qkv"].to(dev), c["dout"].to(dev)
        mask_d = None if c["mask"] is None else c["mask"].to(torch.uint8).to(dev)
        plain_out = ops.attn_pad(qkv_d, mask_d, r, l, h)
        plain_dqkv = _bwd_poisoned(ops, qkv_d, mask_d, dout_d, r, l, h, dh, dev)
        for p in ATTN_P:
            name = f"attn_pad_drop R{r} L{l} H{h} dh{dh} {kind} p={p}"
            cd = _attn_drop_case(r, l, h, dh, kind, p)
            drop = _drop(dev, SEED, ATTN_STEP, ATTN_SITE, p)
            out = ops.attn_pad(qkv_d, mask_d, r, l, h, drop=drop)
            _check(name + " fwd", out, cd["o64"], cd["o32"])
            _zeros_stay_zero(name + " fwd", out, cd["o64"])
            assert torch.equal(_bits(out), _bits(ops.attn_pad(qkv_d, mask_d, r, l, h, drop=drop))), \
                name + ": forward runs differ"
            dqkv = _drop_bwd_poisoned(ops, qkv_d, mask_d, dout_d, r, l, h, dh, drop, dev)
            assert bool(torch.isfinite(dqkv).all()), name + ": an element has no owner, or NaN scratch / LDS was read"
            for i, part in enumerate(("dq", "dk", "dv")):
                sl = slice(i * d, (i + 1) * d)
                _check(f"{name} {part}", dqkv[:, sl], cd["g64"][:, sl], cd["g32"][:, sl])
                _zeros_stay_zero(f"{name} {part}", dqkv[:, sl], cd["g64"][:, sl])
            again = ops.attn_pad_bwd(qkv_d, mask_d, dout_d, r, l, h, drop=drop)
            assert torch.equal(_bits(dqkv), _bits(again)), name + ": backward runs differ"
            nxt = _drop(dev, SEED, ATTN_STEP + 1, ATTN_SITE, p)
            if l > 1:  # one key: 3 * H draws, which two steps can well share
                assert not torch.equal(out, ops.attn_pad(qkv_d, mask_d, r, l, h, drop=nxt)), name + ": step + 1"
                assert not torch.equal(dqkv, ops.attn_pad_bwd(qkv_d, mask_d, dout_d, r, l, h, drop=nxt))
        name = f"attn_pad (after DROP) R{r} L{l} H{h} dh{dh} {kind}"
        out = ops.attn_pad(qkv_d, mask_d, r, l, h)
        dqkv = _bwd_poisoned(ops, qkv_d, mask_d, dout_d, r, l, h, dh, dev)
        assert torch.equal(_bits(out), _bits(plain_out)) and torch.equal(_bits(dqkv), _bits(plain_dqkv)), name
        _check(name + " fwd", out, c["o64"], c["o32"])
        for i, part in enumerate(("dq", "dk", "dv")):
            sl = slice(i * d, (i + 1) * d)
            _check(f"{name} {part}", dqkv[:, sl], c["g64"][:, sl], c["g32"][:, sl])


def test_attn_pad_drop_keeps_the_plain_limits(dev):
    """Same head widths, same L limits as the plain entry points; a missing snapshot is refused; nothing written."""
    from vidsitu_amd import ops

    snap, site, thr, scale = _drop(dev, SEED, 0, 1, 0.1)
    for r, l, h, dh in ((1, 4096, 1, 64), (2, 8, 1, 48), (1, 200, 2, 128)):
        d = h * dh
        qkv = torch.randn(r * l, 3 * d, device=dev)
        out = torch.full((r * l, d), 7.0, device=dev)
        with pytest.raises(ops._lib.VsError):
            ops._lib.call("vs_attn_pad_drop_fwd", ops._ptr(qkv), None, ops._ptr(out), r, l, h, dh, ops._ptr(snap), site,
                          thr, scale, ops._stream())
        dqkv = torch.full((r * l, 3 * d), 7.0, device=dev)
        ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=dev)
        with pytest.raises(ops._lib.VsError):
            ops._lib.call("vs_attn_pad_drop_bwd", ops._ptr(qkv), None, ops._ptr(out), ops._ptr(dqkv), ops._ptr(ws),
                          1 << 62, r, l, h, dh, ops._ptr(snap), site, thr, scale, ops._stream())
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((dqkv == 7.0).all()) and bool((ws == 7).all())
    qkv = torch.randn(16, 3 * 32, device=dev)
    out = torch.full((16, 32), 7.0, device=dev)
    with pytest.raises(ops._lib.VsError):
        ops._lib.call("vs_attn_pad_drop_fwd", ops._ptr(qkv), None, ops._ptr(out), 1, 16, 1, 32, None, site, thr, scale,
                      ops._stream())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------
# the residual site y = LayerNorm(res + m o b) as the models run it: vs_dropout_add_f32 then vs_add_layernorm_fwd on
# the sum; backward vs_add_layernorm_bwd then vs_dropout_add_f32 on ds.  (The pair of kernels that drew the mask
# inside the LayerNorm passes lost against this composition and left with its tests:
# profiles/roberta_dropout_fused_site.json, docs/experiments/roberta_fused_ln_site.patch.)
# ---------------------------------------------------------------------------------------------
# rows 1, 3, 5 (a LayerNorm block holds four rows), 240; D = 64 (synth-tiny), 768 (roberta-base), 6 (the scalar
# kernels of both: D % 4 != 0)
LN_CASES = [(rows, d) for d in (6, 64, 768) for rows in (1, 3, 5, 240)]
LN_STEP, LN_SITE, LN_EPS = 8, 5, 1e-5
LN_KEYS = ("y", "mean", "rstd", "d_b", "d_res", "dgamma", "dbeta")


def _ln_sets(rows):
    """Independent input sets (and steps) per shape: with one row, `mean` is ONE number per run, and the fp32 floor of
    a single number can be 0 by luck; 16 runs make it a floor."""
    return max(1, 16 // rows)


@functools.lru_cache(maxsize=None)
def _ln_case(rows, d, p, k=0):
    """Input set k of a shape, drawn at step LN_STEP + k; fp64 / fp32 references computed once, left unchanged."""
    g = _gen(100 * rows + d + 7919 * k)
    b, res, dy = (torch.randn(rows, d, generator=g) for _ in range(3))
    gamma, beta = 1.0 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    thr, scale = dropout_ref.threshold(p)
    m = torch.from_numpy(dropout_ref.keep_flat(SEED, LN_STEP + k, LN_SITE, rows * d, thr)).double().view(rows, d) * scale
    out = {}
    for dt in (torch.float64, torch.float32):
        bb, rr, gg, be = (t.clone().to(dt).requires_grad_(True) for t in (b, res, gamma, beta))
        y, mean, rstd = dref.add_layernorm(bb, rr, gg, be, LN_EPS, m)
        grads = torch.autograd.grad(y, (bb, rr, gg, be), dy.to(dt))
        out[dt] = dict(y=y.detach(), mean=mean.detach(), rstd=rstd.detach(), d_b=grads[0], d_res=grads[1],
                       dgamma=grads[2], dbeta=grads[3])
    return dict(b=b, res=res, dy=dy, gamma=gamma, beta=beta, m=m, r64=out[torch.float64], r32=out[torch.float32])


def _ln_run(ops, c, drop, dev):
    """Forward and backward of the site as hf_roberta._ln_site / _ln_site_bwd issue them -> the seven results."""
    b, res, dy, gamma, beta = (c[k].to(dev) for k in ("b", "res", "dy", "gamma", "beta"))
    s = ops.dropout_add(b, res, drop)
    y, mean, rstd = ops.add_layernorm_fwd(s, None, gamma, beta, LN_EPS)
    dg, db = torch.full_like(gamma, NAN), torch.full_like(beta, NAN)  # overwrite semantics
    ds = ops.add_layernorm_bwd(dy, s, None, gamma, mean, rstd, dg_out=dg, db_out=db)[0]
    return dict(y=y, mean=mean, rstd=rstd, d_b=ops.dropout_add(ds, None, drop), d_res=ds, dgamma=dg, dbeta=db)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("rows,d", LN_CASES, ids=[f"rows{r}_D{d}" for r, d in LN_CASES])
def test_residual_site_composition(rows, d, p, dev):
    from vidsitu_amd import ops

    name = f"residual site rows{rows} D{d} p={p}"
    cases = [_ln_case(rows, d, p, k) for k in range(_ln_sets(rows))]
    gots = [_ln_run(ops, c, _drop(dev, SEED, LN_STEP + k, LN_SITE, p), dev) for k, c in enumerate(cases)]
    for k in LN_KEYS:  # the rule on each result, over all input sets of the shape together
        _check(f"{name} {k}", torch.stack([g[k] for g in gots]), torch.stack([c["r64"][k] for c in cases]),
               torch.stack([c["r32"][k] for c in cases]))
    dropped = (cases[0]["m"] == 0).to(dev)
    assert bool((gots[0]["d_b"][dropped] == 0).all())


# ---------------------------------------------------------------------------------------------
# the models: roberta-synth-tiny, R = 3, L = 17, right padding
# ---------------------------------------------------------------------------------------------
DIMS = ref.TINY
R, L = 3, 17
N_LOSSES = 8
ARMS = {"hidden": (0.1, 0.0), "attention": (0.0, 0.1), "both": (0.1, 0.1), "both_half": (0.5, 0.5)}


@functools.lru_cache(maxsize=None)
def _batch():
    toks, mask = ref.golden_inputs(DIMS, R, L, 13)
    g = _gen(77)
    labels = torch.randint(0, 5, (N_LOSSES, R), generator=g)
    # several losses over the same outputs: one scalar's fp32 floor can be almost 0 by luck
    wh = torch.randn(N_LOSSES, R, L, DIMS["d_model"], generator=g) / (L * DIMS["d_model"])
    wp = torch.randn(N_LOSSES, R, DIMS["d_model"], generator=g) / DIMS["d_model"]
    return toks, mask, labels, wh, wp


@functools.lru_cache(maxsize=None)
def _weights(kind):
    if kind == "cls":
        return ref.make_weights(DIMS, 31, prefix="roberta.", pooler=False, num_labels=5)
    return ref.make_weights(DIMS, 31)


def _losses(kind, outs, dev=None):
    toks, mask, labels, wh, wp = _batch()
    mv = (lambda t: t) if dev is None else (lambda t: t.to(dev))
    if kind == "cls":
        (logits,) = outs
        if dev is None:
            return [torch.nn.functional.cross_entropy(logits, lb) for lb in labels]
        from vidsitu_amd.mdl_sf_base import hip_cross_entropy

        return [hip_cross_entropy(logits if i == 0 else logits.detach(), mv(lb)) for i, lb in enumerate(labels)]
    hidden, pooled = outs
    dt = hidden.dtype
    live = dev is None  # on the GPU only the first loss keeps the autograd node
    return [((hidden if live or i == 0 else hidden.detach()) * mv(wh[i]).to(dt)).sum()
            + ((pooled if live or i == 0 else pooled.detach()) * mv(wp[i]).to(dt)).sum() for i in range(N_LOSSES)]


@functools.lru_cache(maxsize=None)
def _model_ref(kind, step, p_hid, p_att):
    """[(outputs, losses, {name: grad}) in fp64, the same in fp32] at the model's (seed, step)."""
    toks, mask, *_ = _batch()
    drops = dref.masks(SEED, step, DIMS, R, L, p_hid, p_att, head=kind == "cls")
    res = []
    for dt in (torch.float64, torch.float32):
        w = {k: v.detach().clone().to(dt).requires_grad_(True) for k, v in _weights(kind).items()}
        if kind == "cls":
            h = dref.encoder(w, toks, mask, DIMS, drops, prefix="roberta.")
            outs = (dref.classifier(w, h, drops, DIMS["n_layer"]),)
        else:
            h = dref.encoder(w, toks, mask, DIMS, drops)
            outs = (h, dref.pooler(w, h))
        losses = _losses(kind, outs)
        losses[0].backward()
        grads = {k: v.grad for k, v in w.items()}
        for k in grads:  # nn.Embedding(padding_idx = pad): that row of both tables never receives a gradient
            if "word_embeddings" in k or "position_embeddings" in k:
                grads[k][DIMS["pad_token_id"]] = 0
        res.append((tuple(o.detach() for o in outs), torch.stack([x.detach() for x in losses]), grads))
    return res


def _model(kind, dev, **kw):
    from vidsitu_amd.hf_roberta import RobertaForSequenceClassificationHip, RobertaModelHip

    m = RobertaForSequenceClassificationHip(**DIMS, num_labels=5, **kw) if kind == "cls" else RobertaModelHip(**DIMS, **kw)
    m.load_state_dict({k: v.float() for k, v in _weights(kind).items()}, strict=True)
    return m.to(dev)


def _train_pass(m, dev):
    from vidsitu_amd import hf_roberta

    toks, mask, *_ = _batch()
    return hf_roberta.roberta_apply(m, toks.to(dev), mask.to(dev))


def _check_grad(name, got, ref64, ref32, top):
    """The rule on one parameter gradient; key.bias (analytically zero) on the scale of the model's largest entry."""
    assert got is not None and bool(torch.isfinite(got).all()), f"{name}: missing or non-finite gradient"
    if not name.endswith("attention.self.key.bias"):
        return _check(name, got, ref64, ref32)
    e32 = float((ref32.double() - ref64).abs().max()) / top
    err = float((got.detach().cpu().double() - ref64).abs().max()) / top
    print(f"PARITY {name} (analytically zero; on the model's scale {top:.3e}) e32={e32:.3e} err={err:.3e}")
    assert err <= min(FACTOR * e32, CEILING), f"{name}: kernel error {err:.3e} vs fp32 floor {e32:.3e}"


def _check_model(name, kind, m, outs, step, p_hid, p_att, backward=True):
    (o64, ls64, g64), (o32, ls32, g32) = _model_ref(kind, step, p_hid, p_att)
    dev = outs[0].device
    for what, got, a, b in zip(("logits",) if kind == "cls" else ("hidden", "pooled"), outs, o64, o32):
        _check(f"{name} {what}", got.detach(), a, b)
    losses = _losses(kind, outs, dev)
    _check(f"{name} loss", torch.stack([x.detach() for x in losses]), ls64, ls32)
    if backward:
        for p in m.parameters():
            p.grad = None
        losses[0].backward()
        top = max(float(v.abs().max()) for v in g64.values())
        for k in g64:
            _check_grad(f"{name} grad {k}", m.P(k).grad, g64[k], g32[k], top)


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("kind", ["pool", "cls"])
def test_model_outputs_loss_and_gradients(kind, arm, dev):
    """Hidden only, attention only, both: a site applied in the wrong place, with the wrong probability or the wrong
    element index fails one arm."""
    p_hid, p_att = ARMS[arm]
    m = _model(kind, dev, hidden_dropout_prob=p_hid, attention_probs_dropout_prob=p_att).train()
    step = 6
    m.set_dropout_state((SEED, step))
    outs = _train_pass(m, dev)
    assert m.dropout_state() == (SEED, step + 1)
    _check_model(f"roberta dropout {kind} [{arm}]", kind, m, outs, step, p_hid, p_att)


# ---------------------------------------------------------------------------------------------
# the [seed, step] state
# ---------------------------------------------------------------------------------------------
def _tensors(x):
    if isinstance(x, torch.Tensor):
        return [x]
    return [t for y in x for t in _tensors(y)] if isinstance(x, (tuple, list)) else []


@pytest.mark.parametrize("kind", ["pool", "cls"])
def test_no_mask_tensor_is_saved(kind, dev):
    """What forward_train keeps for the backward at p = 0.1 is what it keeps at p = 0 plus the two-word snapshot."""
    toks, mask, *_ = _batch()
    shapes = []
    for p in (0.0, 0.1):
        m = _model(kind, dev, hidden_dropout_prob=p, attention_probs_dropout_prob=p).train()
        m.forward_train(toks.to(dev), mask.to(dev))
        shapes.append(sorted((str(t.dtype), tuple(t.shape)) for t in _tensors(m.take_train_state())))
    extra = list(shapes[1])
    for s in shapes[0]:
        extra.remove(s)
    assert extra == [("torch.int64", (2,))]
    h = DIMS["n_head"]
    assert not any(s[1] in ((R, h, L, L), (R * h, L, L), (R * h * L, L)) for s in shapes[1])


def test_three_eager_forwards_use_consecutive_steps(dev):
    m = _model("cls", dev, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1).train()
    s = 30
    m.set_dropout_state((SEED, s))
    toks, mask, *_ = _batch()
    for k in range(3):
        outs = m.forward_train(toks.to(dev), mask.to(dev))
        assert m.dropout_state() == (SEED, s + k + 1)
        _check_model(f"roberta dropout [eager forward {k}]", "cls", m, outs, s + k, 0.1, 0.1, backward=False)


def test_graph_replays_of_the_forward_use_consecutive_steps(dev):
    """The tick is captured with the forward: three replays, three different sets of masks, each its step's."""
    m = _model("pool", dev, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1).train()
    toks, mask, *_ = _batch()
    td, md = toks.to(dev), mask.to(dev)
    m.forward_train(td, md)  # eager: the fused q/k/v weights and the state exist before the capture
    s = 50
    m.set_dropout_state((SEED, s))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = m.forward_train(td, md)
    assert m.dropout_state() == (SEED, s), "the capture itself must not advance the state"
    seen = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert m.dropout_state() == (SEED, s + k + 1)
        now = tuple(o.clone() for o in outs)
        _check_model(f"roberta dropout [graph replay {k}]", "pool", m, now, s + k, 0.1, 0.1, backward=False)
        seen.append(now[0])
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_backward_out_of_order_sees_its_own_masks(dev):
    """Two forwards, then the backward of the FIRST: its snapshot travelled with its autograd node."""
    m = _model("cls", dev, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1).train()
    step = 12
    m.set_dropout_state((SEED, step))
    first = _train_pass(m, dev)
    second = _train_pass(m, dev)
    assert m.dropout_state() == (SEED, step + 2)
    assert not torch.equal(first[0], second[0])
    _check_model("roberta dropout [second forward]", "cls", m, second, step + 1, 0.1, 0.1, backward=False)
    _check_model("roberta dropout [first forward, backward after the second]", "cls", m, first, step, 0.1, 0.1)


@pytest.mark.parametrize("kind", ["pool", "cls"])
def test_eval_applies_no_dropout_and_does_not_tick(kind, dev):
    from vidsitu_amd import hf_roberta

    plain = _model(kind, dev).eval()
    m = _model(kind, dev, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1).eval()
    m.set_dropout_state((SEED, 4))
    toks, mask, *_ = _batch()
    td, md = toks.to(dev), mask.to(dev)
    key = "logits" if kind == "cls" else "last_hidden_state"
    assert torch.equal(_bits(m(td, md)[key]), _bits(plain(td, md)[key]))
    assert torch.equal(_bits(hf_roberta.roberta_apply(m, td, md)[0]), _bits(hf_roberta.roberta_apply(plain, td, md)[0]))
    m.train()
    assert torch.equal(_bits(m(td, md)[key]), _bits(plain(td, md)[key]))  # forward() is the inference pass in any mode
    with torch.no_grad():  # train mode without autograd is the inference pass too
        assert torch.equal(_bits(hf_roberta.roberta_apply(m, td, md)[0]),
                           _bits(hf_roberta.roberta_apply(plain, td, md)[0]))
    assert m.dropout_state() == (SEED, 4)


def test_creating_the_state_inside_a_capture_is_refused(dev, monkeypatch):
    """(A capture is answered by a stand-in, as tests/test_flat_module.py does: nothing is captured.)"""
    from vidsitu_amd import _lib

    m = _model("pool", dev, hidden_dropout_prob=0.1).train()
    toks, mask, *_ = _batch()
    m.eval()(toks.to(dev), mask.to(dev))  # the fused q/k/v weights exist; the state does not
    m.train()
    assert m.dropout_state() is None
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.VsError, match="the RoBERTa dropout state must exist before a graph capture"):
        m.forward_train(toks.to(dev), mask.to(dev))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert m.dropout_state() is None


def test_state_is_no_parameter_and_moves_with_the_module(dev):
    m = _model("pool", dev, hidden_dropout_prob=0.1).train()
    assert m.dropout_state() is None
    assert not any("drop" in k for k in m.state_dict()) and not any("drop" in k for k, _ in m.named_buffers())
    torch.manual_seed(123)
    _train_pass(m, dev)
    seed, step = m.dropout_state()
    torch.manual_seed(123)
    assert seed == int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)) and step == 1  # torch.manual_seed governs it
    assert not any("drop" in k for k in m.state_dict()) and len(list(m.parameters())) == len(m._names)
    m = m.to("cpu")
    assert m._drop_state.device.type == "cpu" and m.dropout_state() == (seed, 1)
    m = m.to(dev)
    assert m._drop_state.is_cuda and m.dropout_state() == (seed, 1)


def _grads_after(kind, m, dev):
    from vidsitu_amd import _lib

    for p in m.parameters():
        p.grad = None
    before = _lib.load().vs_launch_count()
    outs = _train_pass(m, dev)
    _losses(kind, outs, dev)[0].backward()
    torch.cuda.synchronize()
    return ([o.detach() for o in outs], {k: m.P(k).grad.clone() for k in m._names},
            _lib.load().vs_launch_count() - before)


def test_set_dropout_state_reproduces_the_next_step(dev):
    m = _model("cls", dev, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1).train()
    _grads_after("cls", m, dev)
    state = m.dropout_state()
    o1, g1, _ = _grads_after("cls", m, dev)
    o2, _, _ = _grads_after("cls", m, dev)
    assert not torch.equal(o1[0], o2[0])
    m.set_dropout_state(state)
    o3, g3, _ = _grads_after("cls", m, dev)
    assert torch.equal(_bits(o1[0]), _bits(o3[0]))
    for k in g1:  # the two embedding tables' backward adds rows with fp32 atomics: summation-order noise
        if "word_embeddings" in k or "position_embeddings" in k:
            assert float((g1[k] - g3[k]).abs().max()) <= 1e-5 * float(g1[k].abs().max()), k
        else:
            assert torch.equal(_bits(g1[k]), _bits(g3[k])), k


@pytest.mark.parametrize("kind", ["pool", "cls"])
def test_train_mode_at_p0_is_the_model_without_the_arguments(kind, dev):
    """Same launches (their count; no tick: the state is never created) and the same bits; the two embedding tables'
    gradients (fp32 atomics where several tokens meet in a row) to summation-order noise."""
    old = _model(kind, dev).train()
    new = _model(kind, dev, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0).train()
    _grads_after(kind, old, dev)  # the fused q/k/v weights exist on both sides from here on
    _grads_after(kind, new, dev)
    oo, go, no = _grads_after(kind, old, dev)
    on, gn, nn_ = _grads_after(kind, new, dev)
    print(f"LAUNCHES {kind}: {no} without the arguments, {nn_} with p = 0")
    assert no == nn_ and new.dropout_state() is None and new._drop_state is None
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(oo, on))
    for k in go:
        if "word_embeddings" in k or "position_embeddings" in k:
            assert float((go[k] - gn[k]).abs().max()) <= 1e-5 * float(go[k].abs().max()), k
        else:
            assert torch.equal(_bits(go[k]), _bits(gn[k])), k


# ---------------------------------------------------------------------------------------------
# the plugin surface
# ---------------------------------------------------------------------------------------------
def _evrel(row, p, dev):
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.hf_roberta import _RobertaHip
    from vidsitu_amd.mdl_sf_base import get_head_dim
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    cfg = get_cfg({"task_type": "evrel", "mdl.mdl_name": row, "mdl.rob_mdl_name": "roberta-synth-tiny",
                   "mdl.rob_dropout": p})
    comm = synth_data.make_comm(cfg)
    sel = get_mdl_loss_eval(cfg)
    torch.manual_seed(0)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev)
    batch = synth_data.synth_evrel_batch(comm, 2, n_ann=1, feat_dim=get_head_dim(cfg), seed=41)
    (rob,) = [x for x in mdl.modules() if isinstance(x, _RobertaHip)]
    return cfg, comm, sel, mdl, rob, {k: v.to(dev) for k, v in batch.items()}


@pytest.mark.parametrize("row", ["rob_evrel", "sfpret_evrel"])
def test_plugin_surface_with_rob_dropout(row, dev):
    """One training step and one validation pass through get_mdl_loss_eval at mdl.rob_dropout = 0.1."""
    from vidsitu_amd.optim import ArenaAdam, ParamArena

    losses = {}
    for p in (0.0, 0.1):
        cfg, comm, sel, mdl, rob, batch = _evrel(row, p, dev)
        assert (rob.hidden_dropout_prob, rob.attention_probs_dropout_prob) == (p, p)
        mdl.train()
        loss_fn = sel["loss"](cfg, comm)
        arena = ParamArena(mdl, adopt_conv=False)
        opt = ArenaAdam(arena, lr=1e-3)
        opt.zero_grad()
        loss = loss_fn(mdl(batch), batch)["loss"]
        loss.backward()
        opt.step()
        losses[p] = float(loss.detach())
        assert rob.dropout_state() == (None if p == 0.0 else (rob.dropout_state()[0], 1))
        mdl.eval()
        with torch.no_grad():
            out = mdl(batch)
            val = float(loss_fn(out, batch)["loss"])
        assert bool(torch.isfinite(out["mdl_out"]).all()) and val == val and abs(val) != float("inf")
        assert bool(torch.isfinite(arena.data).all())
        if p:
            assert rob.dropout_state()[1] == 1, "validation must not tick"
    print(f"{row}: first training loss {losses[0.0]:.6f} at rob_dropout 0, {losses[0.1]:.6f} at 0.1")
    assert all(x == x and abs(x) != float("inf") for x in losses.values()) and losses[0.0] != losses[0.1]


def test_onlyvid_model_allocates_no_dropout_state(dev):
    cfg, comm, sel, mdl, rob, batch = _evrel("sfpret_onlyvid_evrel", 0.1, dev)
    assert rob.hidden_dropout_prob == 0.1
    mdl.train()
    loss = sel["loss"](cfg, comm)(mdl(batch), batch)["loss"]
    loss.backward()
    assert bool(torch.isfinite(loss)) and rob.dropout_state() is None and rob._drop_state is None
