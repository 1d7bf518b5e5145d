"""`GPT2LMHeadModelHip(..., decode_matmul="bf16")`: bf16 weights and operands, fp32 accumulation, in the five dense
projections of the cached decode step; everything else of the step fp32; the default untouched bit for bit.

Kernels (csrc/txenc_ops.hip): vs_pack_rows_bf16 writes the fragment-major bf16 weight image, vs_gemm_nt_bf16_packed
multiplies it with the fp32 activation image (rounded as it is loaded) on v_mfma_f32_16x16x32_bf16.

Reference of the GEMM: `test_gpu_gemm_bf16._restate` -- both operands rounded with `tensor.bfloat16()`, then
act(x w^T + b) + res in fp64; `e32` is the same in fp32.  Rule of tests/test_gpu_gpt2_ops.py, unchanged:
err <= min(16 * e32, 2e-4), both relative to max |fp64|.  Products of bf16 values are exact in fp32, so only the
summation order separates the kernel from the restatement.  x reaches the kernel UNROUNDED.

`CASES` walks the table of shapes: M 1 / 16 / 17 / 33 / 50 / 64 (one to four row blocks, a partial last block), K 128 /
256 / 384 / 1024 / 4096, N 16 / 97 (a partial column tile; 7 tiles, so the early-return blocks of the 8-wide XCD
mapping run) / 384 / 1024, and N 3 040 / 12 193 at K = 128 (the two wide-N branches of the dispatcher: all rows x 16
columns and all rows x 64 columns).  Every tile shape takes every K % 128 == 0 -- a wave owns whole chunks of K and
counts its own groups, waves past K idle -- so the choice depends on M and N alone and the K = 128 cases reach every
plan index (asserted).  With K = 128 only, the two-stage loop of the wide-N shapes would never turn: `EXTRA` adds three
cases beyond the table for that (K = 384: three groups in 4 waves, the odd tail; K = 1024 and 1536 in 8 waves: one trip,
and a partial last group in which waves 4..7 idle).  Between them the cases take every epilogue: bias or none, res,
relu, gelu_new, y_packed.  Every figure is printed (`PARITY ...`) before it is asserted."""
import functools
import os
import re
import subprocess
import sys

import pytest
import torch

import gpt2_bf16_ref as bref
from oracle import gpt2_ref
from test_gemm_bf16_host import NEAR, TIES
from test_gpu_gemm_bf16 import ACT_NAMES, _restate
from test_gpu_gpt2_ops import CEILING, FACTOR, _bits, _errs, _gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (M, N, K, act, bias, res, y_packed)
TABLE = [
    (1, 16, 128, 0, False, False, False),
    (16, 97, 128, 0, True, False, False),
    (17, 97, 256, 1, True, False, False),
    (33, 97, 384, 2, True, True, False),
    (50, 97, 1024, 0, True, True, False),
    (64, 97, 4096, 0, True, False, False),
    (17, 384, 128, 2, True, False, True),
    (50, 384, 1024, 2, True, False, True),
    (64, 384, 384, 0, False, True, False),
    (1, 1024, 1024, 0, True, False, False),
    (50, 1024, 1024, 0, True, True, False),
    (50, 1024, 4096, 0, True, True, False),
    (33, 1024, 256, 1, False, False, False),
    (16, 16, 4096, 0, True, False, True),
    (64, 16, 256, 2, False, True, False),
    (16, 3040, 128, 0, True, False, False),
    (17, 3040, 128, 2, True, False, True),
    (33, 3040, 128, 0, False, True, False),
    (64, 3040, 128, 1, True, True, False),
    (1, 12193, 128, 0, False, False, False),
    (17, 12193, 128, 0, True, False, False),
    (33, 12193, 128, 0, True, True, False),
    (50, 12193, 128, 2, True, False, False),
    (64, 12193, 128, 1, False, True, False),
]
EXTRA = [  # beyond the table: the loops of the wide-N tile shapes (module docstring)
    (50, 12193, 384, 0, False, False, False),
    (33, 3040, 1024, 0, True, False, False),
    (17, 3040, 1536, 2, True, True, True),
]
CASES = TABLE + EXTRA
IDS = [f"M{m}_N{n}_K{k}_{ACT_NAMES[a]}{'_bias' if b else ''}{'_res' if r else ''}{'_ypk' if p else ''}"
       for m, n, k, a, b, r, p in CASES]


def _pad16(n):
    return (n + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def _case(m, n, k, act, bias, res):
    g = _gen(m * 1000003 + n * 1009 + k + 7)
    x, w = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5
    b = torch.randn(n, generator=g) if bias else None
    r = torch.randn(m, n, generator=g) if res else None
    return x, w, b, r, _restate(x, w, b, r, act, torch.float64), _restate(x, w, b, r, act, torch.float32)


def _to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def _check(tag, got, ref64, ref32):
    e32, err = _errs(got, ref64, ref32)
    print(f"PARITY {tag} e32={e32:.3e} err={err:.3e}")
    assert bool(torch.isfinite(got).all()), tag
    assert err <= min(FACTOR * e32, CEILING), f"{tag}: kernel error {err:.3e} vs fp32 floor {e32:.3e}"


# ---------------------------------------------------------------------------------------------
# 1. the weight image
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [32, 128, 1024])
@pytest.mark.parametrize("rows", [1, 16, 17, 97])
def test_pack_rows_bf16_is_the_bf16_cast_in_fragment_order(rows, k, dev):
    from vidsitu_amd import ops

    w = torch.randn(rows, k, generator=_gen(rows * 31 + k)) * torch.logspace(-3, 3, k)
    probes = torch.tensor(TIES + NEAR, dtype=torch.float32)
    w.view(-1)[: probes.numel()] = probes
    img = ops.pack_rows_bf16(w.to(dev))
    assert img.numel() == _pad16(rows) * k and img.element_size() == 2
    full = ops.unpack_rows_bf16(img, _pad16(rows), k).cpu()
    want = w.bfloat16().float()
    same = torch.equal(_bits(full[:rows]), _bits(want))
    print(f"PARITY pack_rows_bf16 R={rows} K={k} bitwise={same} pad_rows_zero={not bool(full[rows:].any())}")
    assert same
    assert full[:rows].reshape(-1)[:4].tolist() == [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6)]  # ties to even
    assert _pad16(rows) == rows or (full[rows:].numel() > 0 and not bool(_bits(full[rows:]).any()))


# ---------------------------------------------------------------------------------------------
# 2. the kernel against its restatement
# ---------------------------------------------------------------------------------------------
def test_every_case_has_a_positive_fp32_floor_and_every_plan_is_taken():
    """On the CPU, before anything goes to the GPU: e32 = 0 would collapse the bound to 0."""
    from vidsitu_amd import _lib

    lib = _lib.load()
    for (m, n, k, act, bias, res, _), name in zip(CASES, IDS):
        _, _, _, _, ref64, ref32 = _case(m, n, k, act, bias, res)
        e32 = float((ref32.double() - ref64).abs().max()) / float(ref64.abs().max())
        assert e32 > 0, name
    plans = [lib.vs_gemm_nt_bf16_packed_plan(m, n, k) for m, n, k, *_ in CASES]
    print(f"PARITY gemm_nt_bf16_packed plans of the cases: {plans}")
    assert set(plans) == set(range(lib.vs_gemm_nt_bf16_packed_plan_count()))
    assert {lib.vs_gemm_nt_bf16_packed_plan(m, n, k) for m, n, k, *_ in TABLE} == set(plans)  # the table alone does
    assert {c[3] for c in CASES} == {0, 1, 2} and {c[4] for c in CASES} == {c[5] for c in CASES} == {True, False}
    assert any(c[6] for c in CASES)


def _run_case(ops, dev, m, n, k, act, bias, res, ypk):
    x, w, b, r, _, _ = _case(m, n, k, act, bias, res)
    x_d, w_d, b_d, r_d = _to(dev, x, w, b, r)
    y = ops.gemm_nt_packed_bf16(ops.pack_rows_f32(x_d), ops.pack_rows_bf16(w_d), m, n, k, b=b_d, res=r_d, act=act,
                                y_packed=ypk)
    return ops.unpack_rows_f32(y, m, n) if ypk else y


@pytest.mark.parametrize("m,n,k,act,bias,res,ypk", CASES, ids=IDS)
def test_gemm_nt_packed_bf16_values(m, n, k, act, bias, res, ypk, dev):
    from vidsitu_amd import _lib, ops

    _, _, _, _, ref64, ref32 = _case(m, n, k, act, bias, res)
    got = _run_case(ops, dev, m, n, k, act, bias, res, ypk)
    assert tuple(got.shape) == (m, n)
    plan = _lib.load().vs_gemm_nt_bf16_packed_plan(m, n, k)
    _check(f"gemm_nt_packed_bf16 M={m} N={n} K={k} plan={plan} act={ACT_NAMES[act]}"
           f"{' bias' if bias else ''}{' res' if res else ''}{' ypk' if ypk else ''}", got, ref64, ref32)


@pytest.mark.parametrize("m,n,k,act,bias,res,ypk", [CASES[10], CASES[22]], ids=[IDS[10], IDS[22]])
def test_gemm_nt_packed_bf16_is_deterministic(m, n, k, act, bias, res, ypk, dev):
    """The partial tiles of the waves are added in wave order: two runs agree bit for bit."""
    from vidsitu_amd import ops

    a = _run_case(ops, dev, m, n, k, act, bias, res, ypk).clone()
    b = _run_case(ops, dev, m, n, k, act, bias, res, ypk)
    same = torch.equal(_bits(a), _bits(b))
    print(f"PARITY gemm_nt_packed_bf16 M={m} N={n} K={k} run twice bitwise={same}")
    assert same


def test_operand_size_check_mirrors_gemm_nt_packed(dev):
    from vidsitu_amd import _lib, ops

    x = ops.pack_rows_f32(torch.zeros(17, 128, device=dev))
    w = ops.pack_rows_bf16(torch.zeros(16, 128, device=dev))
    with pytest.raises(_lib.VsError, match="packed operand too small"):
        ops.gemm_nt_packed_bf16(x, w, 33, 16, 128)
    with pytest.raises(_lib.VsError, match="packed operand too small"):
        ops.gemm_nt_packed_bf16(x, w, 17, 17, 128)


# ---------------------------------------------------------------------------------------------
# 3. the mode in the model
# ---------------------------------------------------------------------------------------------
N_LAYER, D, N_HEAD, N_POS, VOCAB = 2, 128, 4, 64, 97  # the smallest model whose step takes the packed GEMMs
PAD = VOCAB - 1
GEMMS = 4 * N_LAYER + 1


@functools.lru_cache(maxsize=None)
def _weights(d=D, seed=29):
    return {k: torch.from_numpy(v) for k, v in gpt2_ref.make_weights(VOCAB, N_POS, d, N_LAYER, seed).items()}


def _model(dev, d=D, **kw):
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip

    m = GPT2LMHeadModelHip(N_LAYER, d, N_HEAD, N_POS, VOCAB, **kw)
    sd = dict(_weights(d))
    sd["lm_head.weight"] = sd["transformer.wte.weight"]
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


def _tokens(rows, length, seed=3):
    return torch.randint(0, PAD, (rows, length), generator=_gen(seed))


def _cpu(t):
    return None if t is None else t.detach().cpu().clone()


def _recording(monkeypatch):
    from vidsitu_amd import ops

    packed, plain = [], []
    real_p, real_g = ops.gemm_nt_packed_bf16, ops.gemm_nt

    def gemm_nt_packed_bf16(x_packed, w_packed16, m, n, k, b=None, res=None, act=ops.ACT_NONE, y_packed=False):
        y = real_p(x_packed, w_packed16, m, n, k, b=b, res=res, act=act, y_packed=y_packed)
        packed.append(dict(x=_cpu(x_packed), w=_cpu(w_packed16), m=m, n=n, k=k, b=_cpu(b), res=_cpu(res), act=int(act),
                           ypk=bool(y_packed), y=_cpu(y)))
        return y

    def gemm_nt(x, w, b=None, res=None, act=ops.ACT_NONE, out=None, bf16=False):
        plain.append(bool(bf16))
        return real_g(x, w, b, res, act=act, out=out, bf16=bf16)

    monkeypatch.setattr(ops, "gemm_nt_packed_bf16", gemm_nt_packed_bf16)
    monkeypatch.setattr(ops, "gemm_nt", gemm_nt)
    monkeypatch.setattr(ops, "gemm_nt_packed", lambda *a, **kw: pytest.fail("an fp32 packed GEMM ran in bf16 mode"))
    return packed, plain


@pytest.mark.parametrize("rows", [20, 3])
def test_every_gemm_of_the_packed_step_is_the_bf16_kernel_and_matches_its_restatement(rows, dev, monkeypatch):
    from vidsitu_amd import ops
    from vidsitu_amd.hf_gpt2_fseq import KVCacheState

    m = _model(dev, decode_matmul="bf16")
    toks = _tokens(rows, 2).to(dev)
    packed, plain = _recording(monkeypatch)
    st = KVCacheState()
    for t in range(2):
        m.forward_step(toks[:, t].contiguous(), st, max_len=8)
        assert len(packed) == (t + 1) * GEMMS and not plain
    assert not m._wpk and len(m._wpk16) == GEMMS  # the fp32 packed copies are never built in this mode
    for i, c in enumerate(packed):
        x = ops.unpack_rows_f32(c["x"], c["m"], c["k"])
        w = ops.unpack_rows_bf16(c["w"], c["n"], c["k"])
        y = ops.unpack_rows_f32(c["y"], c["m"], c["n"]) if c["ypk"] else c["y"]
        assert c["m"] == rows
        ref64 = _restate(x, w, c["b"], c["res"], c["act"], torch.float64)
        ref32 = _restate(x, w, c["b"], c["res"], c["act"], torch.float32)
        _check(f"gpt2 decode bf16 rows={rows} call {i} N={c['n']} K={c['k']} act={ACT_NAMES[c['act']]}"
               f"{' res' if c['res'] is not None else ''}{' ypk' if c['ypk'] else ''}", y, ref64, ref32)
    assert sorted({c["act"] for c in packed}) == [0, 2] and any(c["ypk"] for c in packed)


@pytest.mark.parametrize("d,rows", [(D, 70), (64, 3), (64, 20), (64, 70)])
def test_rows_or_dimensions_outside_the_packed_step_take_gemm_nt_with_bf16_operands(d, rows, dev, monkeypatch):
    from vidsitu_amd.hf_gpt2_fseq import KVCacheState

    m = _model(dev, d=d, decode_matmul="bf16")
    toks = _tokens(rows, 2).to(dev)
    packed, plain = _recording(monkeypatch)
    st = KVCacheState()
    for t in range(2):
        lg = m.forward_step(toks[:, t].contiguous(), st, max_len=8)
    assert not packed and len(plain) == 2 * GEMMS and all(plain)
    assert bool(torch.isfinite(lg).all()) and not m._wpk16 and not m._wpk


# ---------------------------------------------------------------------------------------------
# 4. end to end against the rounding restatement, loosely
# ---------------------------------------------------------------------------------------------
E2E_ROWS, E2E_LEN = 20, 6


@functools.lru_cache(maxsize=None)
def _e2e_refs():
    toks = _tokens(E2E_ROWS, E2E_LEN, seed=11)
    mask = torch.ones(E2E_ROWS, E2E_LEN, dtype=torch.bool)
    w64 = {k: v.double() for k, v in _weights().items()}
    with torch.no_grad():
        exact = bref.forward(w64, toks, mask, N_LAYER, N_HEAD, rnd=False)
        rounded = bref.forward(w64, toks, mask, N_LAYER, N_HEAD, rnd=True)
    return toks, exact, rounded


def test_step_logits_deviate_from_the_exact_model_as_the_rounding_restatement_does(dev):
    """Step logits at position t are the whole-sequence logits at [:, t] (causal attention, no padding).  `d_ref` =
    deviation of the fp64 model that rounds x and W of every dense layer to bf16 from the exact fp64 model, relative
    to max |exact|; the model's must be within [d_ref / 2, 2 * d_ref] (precedent: tests/test_gpu_gpt2_bf16.py)."""
    from vidsitu_amd.hf_gpt2_fseq import KVCacheState

    toks, exact, rounded = _e2e_refs()
    scale = float(exact.abs().max())
    d_ref = float((rounded - exact).abs().max()) / scale
    figures = {}
    for mode in ("bf16", "fp32"):
        m = _model(dev, decode_matmul=mode)
        st = KVCacheState()
        td = toks.to(dev)
        got = torch.stack([m.forward_step(td[:, t].contiguous(), st, max_len=8).cpu() for t in range(E2E_LEN)], dim=1)
        assert bool(torch.isfinite(got).all())
        figures[mode] = float((got.double() - exact).abs().max()) / scale
        print(f"PARITY gpt2 decode [end to end] decode_matmul={mode} d_ref={d_ref:.3e} dev={figures[mode]:.3e} "
              f"ratio={figures[mode] / d_ref:.3f}")
    assert figures["bf16"] <= 2 * d_ref, f"deviation {figures['bf16']:.3e}, the restatement's is {d_ref:.3e}"
    assert figures["bf16"] >= d_ref / 2, f"deviation {figures['bf16']:.3e} only (restatement {d_ref:.3e}): is the mode on?"


# ---------------------------------------------------------------------------------------------
# 5. the default is what it was
# ---------------------------------------------------------------------------------------------
def test_default_decode_is_untouched_and_the_mode_changes_the_logits(dev):
    from vidsitu_amd.hf_gpt2_fseq import KVCacheState

    old, new = _model(dev), _model(dev, decode_matmul="fp32")
    train16, on = _model(dev, matmul="bf16"), _model(dev, decode_matmul="bf16")
    for rows in (3, 20, 70):
        toks = _tokens(rows, 3, seed=rows).to(dev)
        states = [KVCacheState() for _ in range(4)]
        for t in range(3):
            col = toks[:, t].contiguous()
            lo, ln, lt, lb = (m.forward_step(col, s, max_len=8) for m, s in zip((old, new, train16, on), states))
            assert torch.equal(_bits(lo), _bits(ln)), f"rows {rows} step {t}: decode_matmul='fp32' is not the default"
            assert torch.equal(_bits(lo), _bits(lt)), f"rows {rows} step {t}: matmul='bf16' changed the decode step"
            assert not torch.equal(_bits(lo), _bits(lb)), f"rows {rows} step {t}: the bf16 step gave the fp32 bits"
    first = _tokens(3, 1, seed=5).to(dev)
    want = old.generate_greedy(first, 12, PAD, PAD - 1)
    assert torch.equal(want, new.generate_greedy(first, 12, PAD, PAD - 1))
    assert torch.equal(want, train16.generate_greedy(first, 12, PAD, PAD - 1))
    assert not old._wpk16 and not new._wpk16 and not train16._wpk16


# ---------------------------------------------------------------------------------------------
# 6. search and capture
# ---------------------------------------------------------------------------------------------
def _tx_only(dev, mode="bf16"):
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.hf_gpt2_fseq import GPT2LMHeadModelHip
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    cfg = get_cfg({"task_type": "vb_arg", "mdl.mdl_name": "tx_only", "mdl.tx_dec_type": "gpt2",
                   "mdl.gpt2_mdl_name": "gpt2-synth-d128", "synth.gpt2_vocab": VOCAB, "mdl.gpt2_decode_matmul": mode})
    comm = synth_data.make_comm(cfg)
    torch.manual_seed(0)
    mdl = get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=comm).to(dev).eval()
    gpt2 = [x for x in mdl.modules() if isinstance(x, GPT2LMHeadModelHip)]
    assert len(gpt2) == 1 and gpt2[0].decode_matmul == mode and gpt2[0].d_model == 128
    with torch.no_grad():  # make eos reasonably likely so that hypotheses finish at different steps
        gpt2[0].P("transformer.wte.weight")[comm.gpt2_hf_tok.eos_token_id] *= 3.0
    gpt2[0]._drop_copies()
    return cfg, comm, mdl, gpt2[0]


def test_device_search_equals_host_search_and_replays_repeat_bit_for_bit(dev):
    from vidsitu_amd import synth_data
    from vidsitu_amd.seq_gen import SeqGenCustom

    _, comm, mdl, gpt2 = _tx_only(dev)
    batch = synth_data.synth_srl_batch(comm, bs=1, n_ev=5, seq_len=12, device=dev)  # 5 sentences x beam 4 = 20 rows
    prep = mdl.prepare_prev_toks_inp(batch)
    prompt = prep["dst_toks"][..., :1].contiguous()
    sample = dict(batch, src_tokens=prompt, src_lengths=prep["dst_lens"])  # as Simple_TxDec.forward_gen hands it over
    seen, real = [], gpt2._forward_step_packed
    gpt2._forward_step_packed = lambda h, rows, *a: (seen.append(rows), real(h, rows, *a))[1]
    runs = []
    for device_search in (False, True, True, True):  # host; device: eager, graph capture + replay, replay
        gen = SeqGenCustom([mdl], comm.gpt2_hf_tok, beam_size=4, max_len_b=8, min_len=1, device_search=device_search)
        with torch.no_grad():
            runs.append(gen._generate(sample, prefix_tokens=prompt))
    ses = list(mdl.decoder._vs_search_sessions.values())[-1]
    assert ses.uses == 3 and len(ses.graphs) > 0 and 20 in seen and len(gpt2._wpk16) == GEMMS and not gpt2._wpk
    host, dev0 = runs[0], runs[1]
    for sent in range(5):
        assert [h["tokens"].tolist() for h in host[sent]] == [h["tokens"].tolist() for h in dev0[sent]], sent
        for hh, hd in zip(host[sent], dev0[sent]):
            # the host loop drops finished sentences: its later steps run with fewer rows (tests/test_gpu_gpt2.py holds
            # the two searches to the same tokens and to scores equal to fp32 summation-order noise)
            print(f"PARITY gpt2 decode bf16 [search] sentence {sent} host={float(hh['score']):.7f} "
                  f"device={float(hd['score']):.7f}")
            assert abs(float(hh["score"]) - float(hd["score"])) < 1e-5 * max(1.0, abs(float(hh["score"])))
        for again in runs[2:]:
            for h0, h1 in zip(dev0[sent], again[sent]):
                assert torch.equal(h0["tokens"], h1["tokens"])
                assert float(h0["score"]) == float(h1["score"])
                assert torch.equal(_bits(h0["positional_scores"]), _bits(h1["positional_scores"]))


def test_weight_images_are_not_built_inside_a_capture(dev, monkeypatch):
    """(A capture is answered by a stand-in, as tests/test_flat_module.py does: nothing is captured.)"""
    from vidsitu_amd import _lib
    from vidsitu_amd.hf_gpt2_fseq import KVCacheState

    m = _model(dev, decode_matmul="bf16")
    col = _tokens(20, 1).to(dev)[:, 0].contiguous()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.VsError) as err:
        m.forward_step(col, KVCacheState(), max_len=8)
    assert str(err.value) == m._CAPTURE_MSG and not m._wpk16
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    m.forward_step(col, KVCacheState(), max_len=8)  # the eager step builds them ...
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    m.forward_step(col, KVCacheState(), max_len=8)  # ... and a capture is then served from the cache
    assert len(m._wpk16) == GEMMS


# ---------------------------------------------------------------------------------------------
# 7. plugin surface
# ---------------------------------------------------------------------------------------------
def test_main_dist_generates_with_bf16_decode_weights(dev, tmp_path):
    """`python main_dist.py <uid> ... --mdl.tx_dec_type=gpt2 --mdl.gpt2_decode_matmul=bf16` in a fresh child process,
    as a user's run is: it trains, validates (one beam search per batch) and reports the mode the model holds."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "main_dist.py", "t_gpt2_dec16", "--task_type=vb_arg", "--mdl.mdl_name=tx_only",
           "--mdl.tx_dec_type=gpt2", "--mdl.gpt2_mdl_name=gpt2-synth-d128", "--synth.gpt2_vocab=97",
           "--mdl.gpt2_decode_matmul=bf16", "--train.bs=2", "--ds.vsitu.num_ev=2", "--train.lr=1e-3",
           "--overfit_batch=True", "--gen.beam_size=2", "--gen.max_len_b=8", f"--misc.tmp_path={tmp_path}", "--steps=2"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    err = "\n".join(ln for ln in r.stderr.splitlines() if "frame #" not in ln)[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + err
    print(r.stdout[-1500:])
    assert "GPT-2 decoder: matmul fp32, decode_matmul bf16" in r.stdout, r.stdout
    m = re.search(r"'generated_sequences': (\d+)", r.stdout)
    assert m and int(m.group(1)) == 4, r.stdout  # 2 videos x 2 events
