"""Train-mode dropout of the GPT-2 decoder from the in-kernel counter generator (csrc/dropout_rng.h).

Masks come from the CPU restatement (tests/dropout_ref.py); values are held to the rule of tests/test_gpu_gpt2_ops.py:
kernel error <= min(16 * e32, 2e-4) against an fp64 torch restatement with mask operands, e32 = the same
restatement's fp32 noise floor, both relative to max |fp64| (parameter gradients: ceiling 5e-4, that of the
existing gradient test).  Every figure is printed (`PARITY ...`) before it is asserted.
"""
import functools

import numpy as np
import pytest
import torch

import dropout_ref
import gpt2_dropout_ref as gref
from oracle import gpt2_ref
from test_gpu_gpt2_ops import ATTN_CASES, _bits, _check, _errs, _gen, _key_mask

pytestmark = pytest.mark.gpu

NAN = float("nan")
FACTOR = 16.0
GRAD_CEILING = 5e-4
SEED = (0x51ed << 32) | 0x2705a3c9  # above 2^32: both key words in play


def _snap(dev, seed, step):
    return torch.tensor([seed, step], dtype=torch.int64, device=dev)


def _drop(dev, seed, step, site, p):
    from vidsitu_amd import ops

    return (_snap(dev, seed, step), site) + ops.dropout_params(p)


# ---------------------------------------------------------------------------------------------
# vs_dropout_add_f32, vs_dropout_tick
# ---------------------------------------------------------------------------------------------
# 1 / 3 / 1023 / 4097: the scalar kernel (n % 4 != 0), one and several blocks; 4 / 4096 / 8192: the 16-byte kernel,
# one thread, exactly four blocks, eight.  The kernels have no grid-stride loop: the grid covers n.
MASK_N = [1, 3, 4, 1023, 4096, 4096 + 1, 8192]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n", MASK_N)
def test_dropout_add_mask_is_the_reference_pattern(n, p, dev):
    """x = 1, res = None: the output is exactly {0, scale} in the reference's pattern; a NaN-filled output and the
    sentinels around it show every element written and nothing else."""
    from vidsitu_amd import ops

    step, site = 5, 3
    drop = _drop(dev, SEED, step, site, p)
    thr, scale = drop[2], drop[3]
    assert (thr, scale) == dropout_ref.threshold(p)
    want = torch.from_numpy(dropout_ref.keep_flat(SEED, step, site, n, thr)).float() * scale
    buf = torch.full((n + 8,), NAN, device=dev)
    ops.dropout_add(torch.ones(n, device=dev), None, drop, out=buf[4:4 + n])
    assert torch.equal(buf[4:4 + n].cpu(), want)
    assert bool(torch.isnan(buf[:4]).all()) and bool(torch.isnan(buf[4 + n:]).all())


@pytest.mark.parametrize("which", ["x", "out", "res"])
def test_dropout_add_pointer_off_the_16_byte_grid_takes_the_scalar_kernel(which, dev):
    from vidsitu_amd import ops

    n, p, step, site = 4096, 0.1, 2, 7
    drop = _drop(dev, SEED, step, site, p)
    keep = torch.from_numpy(dropout_ref.keep_flat(SEED, step, site, n, drop[2])).float() * drop[3]

    def tensor(off, fill):
        flat = torch.full((n + 8,), fill, device=dev)
        t = flat[off:off + n]
        assert t.data_ptr() % 16 == (4 * off) % 16
        return flat, t

    _, x = tensor(1 if which == "x" else 0, 1.0)
    _, res = tensor(1 if which == "res" else 0, 2.0)
    flat, out = tensor(1 if which == "out" else 4, NAN)
    ops.dropout_add(x, res, drop, out=out)
    assert torch.equal(out.cpu(), keep + 2.0)
    assert int(torch.isnan(flat).sum()) == 8


@pytest.mark.parametrize("n", [3, 1023, 4096, 12288 + 4])
def test_dropout_add_values(n, dev):
    """Random x and res against res + m * x in fp64 (not bit for bit: the compiler may contract the multiply-add)."""
    from vidsitu_amd import ops

    p, step, site = 0.1, 9, 4
    g = _gen(n)
    x, res = torch.randn(n, generator=g), torch.randn(n, generator=g)
    drop = _drop(dev, SEED, step, site, p)
    m = torch.from_numpy(dropout_ref.keep_flat(SEED, step, site, n, drop[2])).double() * drop[3]
    got = ops.dropout_add(x.to(dev), res.to(dev), drop)
    _check(f"dropout_add n={n} res", got, res.double() + m * x.double(), res + m.float() * x)
    got = ops.dropout_add(x.to(dev), None, drop)
    _check(f"dropout_add n={n}", got, m * x.double(), m.float() * x)
    assert bool((got[(m == 0).to(dev)] == 0).all())


def _mask_of(ops, snap, site, p, n):
    thr, scale = ops.dropout_params(p)
    return ops.dropout_add(torch.ones(n, device=snap.device), None, (snap, site, thr, scale))


def test_tick_advances_the_step_and_snapshots_it(dev):
    """Three eager ticks: the snapshots hold steps s, s+1, s+2 and the masks drawn from them are those steps'."""
    from vidsitu_amd import ops

    s, n, p, site = 41, 1000, 0.5, 2
    thr, scale = dropout_ref.threshold(p)
    state = _snap(dev, SEED, s)
    for k in range(3):
        snap = ops.dropout_tick(state)
        assert snap.tolist() == [SEED, s + k] and state.tolist() == [SEED, s + k + 1]
        want = torch.from_numpy(dropout_ref.keep_flat(SEED, s + k, site, n, thr)).float() * scale
        assert torch.equal(_mask_of(ops, snap, site, p, n).cpu(), want)


def test_tick_inside_a_captured_graph_draws_a_new_mask_every_replay(dev):
    from vidsitu_amd import ops

    s, n, p, site = 7, 1000, 0.5, 1
    thr, scale = dropout_ref.threshold(p)
    state = _snap(dev, SEED, s)
    ones, out = torch.ones(n, device=dev), torch.empty(n, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        snap = ops.dropout_tick(state)
        ops.dropout_add(ones, None, (snap, site, thr, scale), out=out)
    assert state.tolist() == [SEED, s], "the capture itself must not advance the state"
    seen = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        want = torch.from_numpy(dropout_ref.keep_flat(SEED, s + k, site, n, thr)).float() * scale
        assert torch.equal(out.cpu(), want), f"replay {k}"
        seen.append(out.cpu().clone())
    assert state.tolist() == [SEED, s + 3]
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not torch.equal(seen[0], seen[2])


# ---------------------------------------------------------------------------------------------
# causal attention with dropout on the probabilities
# ---------------------------------------------------------------------------------------------
# one key / the 16-query chunk edge / more than 64 keys / L % 4 != 0 / dh 16..64 / left padding
DROP_ATTN = [c for c in ATTN_CASES if c in [(2, 1, 2, 16, "none"), (2, 16, 2, 16, "none"), (2, 17, 3, 32, "right"),
                                            (2, 60, 2, 64, "right"), (1, 65, 2, 64, "none"), (1, 130, 1, 16, "right"),
                                            (3, 24, 2, 64, "left")]]
assert len(DROP_ATTN) == 7
DROP_ATTN_P = [(c, 0.1) for c in DROP_ATTN] + [((2, 17, 3, 32, "right"), 0.5)]
ATTN_STEP, ATTN_SITE = 3, 4


@functools.lru_cache(maxsize=None)
def _attn_case(r, l, h, dh, kind, p):
    g = _gen(11 + 1000 * l + dh)
    d = h * dh
    qkv = torch.randn(r * l, 3 * d, generator=g)
    dout = torch.randn(r * l, d, generator=g)
    mask = _key_mask(kind, r, l)
    fm = torch.zeros(r, l, dtype=torch.bool) if mask is None else mask.long().cumsum(1) == 0
    dout[fm.reshape(-1)] = 0.0  # fully masked queries carry no loss in training (as the plain test does)
    thr, scale = dropout_ref.threshold(p)
    keep = torch.from_numpy(dropout_ref.keep_attn(SEED, ATTN_STEP, ATTN_SITE, r, h, l, thr)).double() * scale
    q64 = qkv.double().requires_grad_(True)
    out64 = gref.attention(q64, mask, r, l, h, dh, keep)
    g64, = torch.autograd.grad(out64, q64, dout.double())
    q32 = qkv.clone().requires_grad_(True)
    out32 = gref.attention(q32, mask, r, l, h, dh, keep)
    g32, = torch.autograd.grad(out32, q32, dout)
    return dict(qkv=qkv, dout=dout, mask=mask, fm=fm.reshape(-1), out64=out64.detach(), out32=out32.detach(),
                g64=g64, g32=g32, keep=keep)


def _attn_drop_bwd_poisoned(ops, qkv_d, mask_d, dout_d, r, l, h, dh, drop, dev):
    """vs_attn_causal_drop_bwd through the C ABI with dqkv and the whole scratch workspace full of NaN."""
    need = ops._lib.load().vs_attn_causal_bwd_scratch_bytes(r, l, h)
    ws = ops._workspace(need, dev)
    ws.view(torch.float32).fill_(NAN)
    dqkv = torch.full_like(qkv_d, NAN)
    snap, site, thr, scale = drop
    ops._lib.call("vs_attn_causal_drop_bwd", ops._ptr(qkv_d), ops._ptr(mask_d), ops._ptr(dout_d), ops._ptr(dqkv),
                  ops._ptr(ws), ws.numel(), r, l, h, dh, ops._ptr(snap), site, thr, scale, ops._stream())
    return dqkv


@pytest.mark.parametrize("case,p", DROP_ATTN_P, ids=[f"R{c[0]}_L{c[1]}_H{c[2]}_dh{c[3]}_{c[4]}_p{p}" for c, p in DROP_ATTN_P])
def test_attn_causal_drop_fwd_bwd(case, p, dev):
    from vidsitu_amd import ops

    r, l, h, dh, kind = case
    c = _attn_case(r, l, h, dh, kind, p)
    d = h * dh
    name = f"attn_causal_drop R{r} L{l} H{h} dh{dh} {kind} p={p}"
    qkv_d, dout_d = c["qkv"].to(dev), c["dout"].to(dev)
    mask_d = None if c["mask"] is None else c["mask"].to(dev)
    drop = _drop(dev, SEED, ATTN_STEP, ATTN_SITE, p)
    # forward
    out = ops.attn_causal(qkv_d, mask_d, r, l, h, drop=drop)
    assert bool(torch.isfinite(out).all())
    ok = ~c["fm"]
    _check(name + " fwd", out[ok.to(dev)], c["out64"][ok], c["out32"][ok])
    assert torch.equal(out, ops.attn_causal(qkv_d, mask_d, r, l, h, drop=drop)), "two forward runs differ"
    # backward: dq, dk, dv separately, NaN-filled dqkv and scratch
    dqkv = _attn_drop_bwd_poisoned(ops, qkv_d, mask_d, dout_d, r, l, h, dh, drop, dev)
    assert bool(torch.isfinite(dqkv).all()), "an element of dqkv has no owner, or NaN scratch / LDS was read"
    for i, part in enumerate(("dq", "dk", "dv")):
        sl = slice(i * d, (i + 1) * d)
        _check(f"{name} {part}", dqkv[:, sl], c["g64"][:, sl], c["g32"][:, sl])
    again = ops.attn_causal_bwd(qkv_d, mask_d, dout_d, r, l, h, drop=drop)
    assert torch.equal(dqkv, again), "two backward runs differ (the kernel claims a fixed summation order)"
    # thr = 0 (p = 0): the _drop entry points are the plain ones bit for bit
    keep_all = (drop[0], drop[1], 0, 1.0)
    assert torch.equal(_bits(ops.attn_causal(qkv_d, mask_d, r, l, h, drop=keep_all)),
                       _bits(ops.attn_causal(qkv_d, mask_d, r, l, h)))
    assert torch.equal(_bits(ops.attn_causal_bwd(qkv_d, mask_d, dout_d, r, l, h, drop=keep_all)),
                       _bits(ops.attn_causal_bwd(qkv_d, mask_d, dout_d, r, l, h)))


# ---------------------------------------------------------------------------------------------
# the model: gpt2-synth-tiny, R = 3, L = 19, one right-padded row
# ---------------------------------------------------------------------------------------------
N_LAYER, D, N_HEAD, N_POS, VOCAB = 2, 64, 4, 64, 97
PAD = VOCAB - 1
R, L = 3, 19
N_LABEL_SETS = 8


@functools.lru_cache(maxsize=None)
def _weights():
    w = gpt2_ref.make_weights(VOCAB, N_POS, D, N_LAYER, 23)
    return {k: torch.from_numpy(v) for k, v in w.items()}


@functools.lru_cache(maxsize=None)
def _batch():
    g = _gen(77)
    toks = torch.randint(0, PAD, (R, L), generator=g)
    toks[1, L - 5:] = PAD  # one right-padded row
    # the loss of several label sets over the same logits: one scalar's fp32 floor can be almost 0 by luck
    labels = [toks] + [torch.where(toks == PAD, toks, torch.randint(0, PAD, (R, L), generator=g))
                       for _ in range(N_LABEL_SETS - 1)]
    return toks, labels


def _model(dev, **pdrop):
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip

    m = GPT2LMHeadModelHip(N_LAYER, D, N_HEAD, N_POS, VOCAB, **pdrop)
    sd = dict(_weights())
    sd["lm_head.weight"] = sd["transformer.wte.weight"]
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def _train_pass(m, toks_d):
    from vidsitu_amd.hf_gpt2_fseq import _GPT2TrainFn

    tick = torch.zeros(1, device=toks_d.device, requires_grad=True)
    return _GPT2TrainFn.apply(m, toks_d, toks_d.ne(PAD), tick)


@functools.lru_cache(maxsize=None)
def _model_ref(step, p_embd, p_attn, p_resid):
    toks, labels = _batch()
    drops = gref.masks(SEED, step, N_LAYER, R, L, D, N_HEAD, p_embd, p_attn, p_resid)
    key_mask = toks.ne(PAD)
    return [gref.run(_weights(), toks, key_mask, N_LAYER, N_HEAD, drops, PAD, labels, dt)
            for dt in (torch.float64, torch.float32)]


def _check_grad(name, got, ref64, ref32):
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite gradient"
    e32, err = _errs(got, ref64, ref32)
    print(f"PARITY {name} e32={e32:.3e} err={err:.3e}")
    assert err <= min(FACTOR * e32, GRAD_CEILING), f"{name}: kernel error {err:.3e} vs fp32 floor {e32:.3e}"


def _check_model(name, m, logits, step, p_embd, p_attn, p_resid, backward=True):
    """logits (of a forward at `step`), the losses of every label set, and (after the backward of the first
    loss) every parameter gradient, against the restatement with that step's masks."""
    from vidsitu_amd.hf_gpt2_fseq import lm_loss

    (lg64, ls64, g64), (lg32, ls32, g32) = _model_ref(step, p_embd, p_attn, p_resid)
    toks, labels = _batch()
    dev = logits.device
    _check(f"{name} logits", logits.detach(), lg64, lg32)
    losses = [lm_loss(logits if i == 0 else logits.detach(), lb.to(dev), PAD) for i, lb in enumerate(labels)]
    _check(f"{name} loss", torch.stack([x.detach() for x in losses]), ls64, ls32)
    if backward:
        for p in m.parameters():
            p.grad = None
        losses[0].backward()
        for k in g64:
            _check_grad(f"{name} grad {k}", m.P(k).grad, g64[k], g32[k])


ARMS = {"all": (0.1, 0.1, 0.1), "embd": (0.1, 0.0, 0.0), "attn": (0.0, 0.1, 0.0), "resid": (0.0, 0.0, 0.1)}


@pytest.mark.parametrize("arm", list(ARMS))
def test_model_logits_loss_and_gradients(arm, dev):
    """All three probabilities at 0.1 and each alone: a site applied in the wrong place or with the wrong element
    index fails one arm."""
    pe, pa, pr = ARMS[arm]
    m = _model(dev, embd_pdrop=pe, attn_pdrop=pa, resid_pdrop=pr).train()
    step = 6
    m.set_dropout_state((SEED, step))
    toks, _ = _batch()
    logits = _train_pass(m, toks.to(dev))
    assert m.dropout_state() == (SEED, step + 1)
    _check_model(f"gpt2 dropout [{arm}]", m, logits, step, pe, pa, pr)


def _tensors(x):
    if isinstance(x, torch.Tensor):
        return [x]
    return [t for y in x for t in _tensors(y)] if isinstance(x, (tuple, list)) else []


def test_no_mask_tensor_is_saved(dev):
    """What forward_train keeps for the backward at p = 0.1 is what it keeps at p = 0 plus the two-word snapshot."""
    toks, _ = _batch()
    td = toks.to(dev)
    shapes = []
    for pdrop in (0.0, 0.1):
        m = _model(dev, embd_pdrop=pdrop, attn_pdrop=pdrop, resid_pdrop=pdrop).train()
        m.forward_train(td, td.ne(PAD))
        shapes.append(sorted((str(t.dtype), tuple(t.shape)) for t in _tensors(m.take_train_state())))
    extra = list(shapes[1])
    for s in shapes[0]:
        extra.remove(s)
    assert extra == [("torch.int64", (2,))]


def test_three_eager_forwards_use_consecutive_steps(dev):
    m = _model(dev, embd_pdrop=0.1, attn_pdrop=0.1, resid_pdrop=0.1).train()
    s = 30
    m.set_dropout_state((SEED, s))
    toks, _ = _batch()
    td = toks.to(dev)
    for k in range(3):
        logits = m.forward_train(td, td.ne(PAD))
        assert m.dropout_state() == (SEED, s + k + 1)
        _check_model(f"gpt2 dropout [eager forward {k}]", m, logits, s + k, 0.1, 0.1, 0.1, backward=False)


def test_graph_replays_of_the_forward_use_consecutive_steps(dev):
    """The tick is captured with the forward: three replays, three different sets of masks, each its step's."""
    m = _model(dev, embd_pdrop=0.1, attn_pdrop=0.1, resid_pdrop=0.1).train()
    toks, _ = _batch()
    td = toks.to(dev)
    mask = td.ne(PAD)
    m.forward_train(td, mask)  # eager: the weight copies and the state exist before the capture
    s = 50
    m.set_dropout_state((SEED, s))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        logits = m.forward_train(td, mask)
    assert m.dropout_state() == (SEED, s), "the capture itself must not advance the state"
    seen = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert m.dropout_state() == (SEED, s + k + 1)
        _check_model(f"gpt2 dropout [graph replay {k}]", m, logits.clone(), s + k, 0.1, 0.1, 0.1, backward=False)
        seen.append(logits.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_backward_out_of_order_sees_its_own_masks(dev):
    """Two forwards, then the backward of the FIRST: its snapshot travelled with its autograd node."""
    m = _model(dev, embd_pdrop=0.1, attn_pdrop=0.1, resid_pdrop=0.1).train()
    step = 12
    m.set_dropout_state((SEED, step))
    toks, _ = _batch()
    first = _train_pass(m, toks.to(dev))
    second = _train_pass(m, toks.to(dev))
    assert m.dropout_state() == (SEED, step + 2)
    assert not torch.equal(first, second)
    _check_model("gpt2 dropout [second forward]", m, second, step + 1, 0.1, 0.1, 0.1, backward=False)
    _check_model("gpt2 dropout [first forward, backward after the second]", m, first, step, 0.1, 0.1, 0.1)


def test_eval_applies_no_dropout_and_does_not_tick(dev):
    from vidsitu_amd.hf_gpt2_fseq import HuggingFaceGPT2Decoder, KVCacheState

    plain = _model(dev).eval()
    m = _model(dev, embd_pdrop=0.1, attn_pdrop=0.1, resid_pdrop=0.1).eval()
    m.set_dropout_state((SEED, 4))
    toks, _ = _batch()
    td = toks.to(dev)
    assert torch.equal(_bits(m.forward_logits(td, td.ne(PAD))), _bits(plain.forward_logits(td, td.ne(PAD))))
    first = td[:, :1].contiguous()
    assert torch.equal(m.generate_greedy(first, 12, PAD, PAD - 1), plain.generate_greedy(first, 12, PAD, PAD - 1))
    sa, sb = KVCacheState(), KVCacheState()
    assert torch.equal(_bits(m.forward_step(first[:, 0].contiguous(), sa, max_len=8)),
                       _bits(plain.forward_step(first[:, 0].contiguous(), sb, max_len=8)))
    dec = HuggingFaceGPT2Decoder.__new__(HuggingFaceGPT2Decoder)
    torch.nn.Module.__init__(dec)
    dec.model, dec.pad_idx = m, PAD
    dec.eval()
    assert torch.equal(_bits(dec(td)[0]), _bits(plain.forward_logits(td, td.ne(PAD))))
    dec.train()
    with torch.no_grad():  # train mode without autograd is the inference pass too
        assert torch.equal(_bits(dec(td)[0]), _bits(plain.forward_logits(td, td.ne(PAD))))
    assert m.dropout_state() == (SEED, 4)


def _grads_after(m, toks_d):
    from vidsitu_amd.hf_gpt2_fseq import lm_loss
    from vidsitu_amd import _lib

    for p in m.parameters():
        p.grad = None
    before = _lib.load().vs_launch_count()
    logits = _train_pass(m, toks_d)
    lm_loss(logits, toks_d, PAD).backward()
    torch.cuda.synchronize()
    return logits.detach(), {k: m.P(k).grad.clone() for k in m._names}, _lib.load().vs_launch_count() - before


def test_train_mode_at_p0_is_the_model_without_the_arguments(dev):
    """Same launches (their count; no tick: the state is never created) and the same bits.  The embedding backward
    adds rows with fp32 atomics, whose order is not fixed where several tokens meet in one row of dwte / dwpe: those
    two gradients are compared bit for bit on a one-row batch of distinct tokens and to summation-order noise on the
    three-row batch."""
    old, new = _model(dev).train(), _model(dev, embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0).train()
    toks, _ = _batch()
    one_row = torch.randperm(PAD, generator=_gen(5))[:L].view(1, L)
    for name, t in (("R3", toks), ("R1 distinct tokens", one_row)):
        td = t.to(dev)
        _grads_after(old, td)  # the transposed weight copies exist on both sides from here on
        _grads_after(new, td)
        lo, go, no = _grads_after(old, td)
        ln, gn, nn_ = _grads_after(new, td)
        print(f"LAUNCHES {name}: {no} without the arguments, {nn_} with p = 0")
        assert no == nn_ and new.dropout_state() is None
        assert torch.equal(_bits(lo), _bits(ln))
        for k in go:
            atomics = k in ("transformer.wte.weight", "transformer.wpe.weight") and t.shape[0] > 1
            if atomics:
                assert float((go[k] - gn[k]).abs().max()) <= 1e-5 * float(go[k].abs().max()), k
            else:
                assert torch.equal(_bits(go[k]), _bits(gn[k])), k


def test_state_is_no_parameter_and_moves_with_the_module(dev):
    m = _model(dev, resid_pdrop=0.1).train()
    assert m.dropout_state() is None
    assert not any("drop" in k for k in m.state_dict()) and not any("drop" in k for k, _ in m.named_buffers())
    toks, _ = _batch()
    td = toks.to(dev)
    torch.manual_seed(123)
    _train_pass(m, td)
    seed, step = m.dropout_state()
    torch.manual_seed(123)
    assert seed == int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)) and step == 1  # torch.manual_seed governs it
    m = m.to("cpu")
    assert m._drop_state.device.type == "cpu" and m.dropout_state() == (seed, 1)
    m = m.to(dev)
    assert m._drop_state.is_cuda and m.dropout_state() == (seed, 1)


def test_plugin_surface_tx_only_with_gpt2_dropout(dev):
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval
    from vidsitu_amd.optim import ArenaAdam, ParamArena

    cfg = get_cfg({"task_type": "vb_arg", "mdl.mdl_name": "tx_only", "mdl.tx_dec_type": "gpt2",
                   "mdl.gpt2_mdl_name": "gpt2-synth-tiny", "synth.gpt2_vocab": 97, "mdl.gpt2_dropout": 0.1})
    comm = synth_data.make_comm(cfg)
    sel = get_mdl_loss_eval(cfg)
    torch.manual_seed(0)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev).train()
    gpt2 = [x for x in mdl.modules() if isinstance(x, GPT2LMHeadModelHip)]
    assert len(gpt2) == 1 and (gpt2[0].embd_pdrop, gpt2[0].attn_pdrop, gpt2[0].resid_pdrop) == (0.1, 0.1, 0.1)
    gpt2 = gpt2[0]
    loss_fn = sel["loss"](cfg, comm)
    batch = synth_data.synth_srl_batch(comm, bs=2, n_ev=5, seq_len=12, device=dev)
    gpt2.set_dropout_state((SEED, 0))
    first = loss_fn(mdl(batch), batch)["loss"].detach().clone()
    second = loss_fn(mdl(batch), batch)["loss"].detach().clone()
    assert float(first) != float(second) and gpt2.dropout_state() == (SEED, 2)
    gpt2.set_dropout_state((SEED, 0))
    again = loss_fn(mdl(batch), batch)["loss"].detach().clone()
    assert torch.equal(_bits(again.reshape(1)), _bits(first.reshape(1)))
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
    print(f"tx_only with gpt2_dropout = 0.1: eval loss {before:.4f} -> {after:.4f} after six Adam steps")
    assert np.isfinite(after) and after < before
