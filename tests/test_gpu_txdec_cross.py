"""The decoder's encoder attention over source sequences (S > 1), the text-mode encoder and the `txed_only` row on the
GPU, against the restatement tests/txdec_cross_ref.py (held to torch.nn.TransformerDecoderLayer in
tests/test_txdec_cross_host.py; fairseq parity is unpinned, as oracle/txdec_ref.py says).
Tolerances are those of tests/test_gpu_txdec.py: logits 2e-4 and gradients 5e-4 of the reference's max (a gradient
whose true value is zero -- k_proj.bias -- on the scale of 1e-3 of the model's largest gradient), loss 1e-4 relative."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import txdec_cross_ref as ref
from oracle import txdec_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOC, FFN, NL, OUT, PAD = ref.VOC, ref.FFN, ref.NL, ref.OUT, ref.PAD
ROWS, L = 5, 9


def _model(dev, w, d, heads):
    from vidsitu_amd.fseq_txdec import TransformerDecoderHip

    m = TransformerDecoderHip(VOC, d, FFN, heads, NL, OUT, PAD, dropout=0.0, max_positions=64)
    m.load_state_dict(w, strict=True)
    return m.to(dev)


def _tokens(seed=0):
    t = torch.randint(0, VOC - 1, (ROWS, L), generator=torch.Generator().manual_seed(seed))
    t[0, 6:] = PAD
    t[3, 4:] = PAD
    return t


def _source(s, d, seed):
    """enc [S, ROWS, d] and its padding mask: right-padded sources of differing lengths, the last one ALL padding."""
    enc = torch.randn(s, ROWS, d, generator=torch.Generator().manual_seed(seed))
    lens = [s, max(1, s - 1), max(1, s // 2), 1, 0]
    return enc, torch.arange(s)[None, :] >= torch.tensor(lens)[:, None]


@functools.lru_cache(maxsize=None)
def _case(d, heads, s):
    """Weights, inputs and the restatement's logits, loss and autograd gradients; computed once, left unchanged."""
    w = txdec_ref.make_weights(VOC, d, FFN, NL, OUT, PAD, seed=3)
    toks = _tokens(seed=2)
    enc, pad_mask = _source(s, d, seed=5 + s)
    wg = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    enc_g = enc.clone().requires_grad_(True)
    logits = ref.decoder_forward(wg, toks, enc_g, pad_mask, PAD, heads, NL)
    loss = txdec_ref.lm_loss(logits, toks, PAD)
    loss.backward()
    return dict(w=w, toks=toks, enc=enc, pad_mask=pad_mask, logits=logits.detach(), loss=float(loss),
                grads={k: v.grad for k, v in wg.items()}, denc=enc_g.grad)


@pytest.mark.parametrize("s", [2, 5, 17])
@pytest.mark.parametrize("d,heads", [(64, 4), (256, 2)], ids=["dh16", "dh128"])
def test_logits_and_gradients_match_the_restatement(d, heads, s, dev):
    from vidsitu_amd.flat_module import FlatTrainFn
    from vidsitu_amd.hf_gpt2_fseq import lm_loss

    c = _case(d, heads, s)
    m = _model(dev, c["w"], d, heads)
    toks, want = c["toks"], c["logits"]
    got = m.eval().forward_logits(toks.to(dev), c["enc"].to(dev), c["pad_mask"].to(dev)).cpu()
    err = float((got - want)[toks.ne(PAD)].abs().max()) / float(want.abs().max())
    print(f"PARITY txdec_cross d{d} S{s} logits err={err:.3e}")
    assert err < 2e-4, err
    m.train()
    enc_d = c["enc"].to(dev).requires_grad_(True)
    tick = torch.zeros(1, device=dev, requires_grad=True)
    logits = FlatTrainFn.apply(m, toks.to(dev), enc_d, c["pad_mask"].to(dev), tick)
    loss = lm_loss(logits, toks.to(dev), PAD)
    print(f"PARITY txdec_cross d{d} S{s} loss {float(loss):.6f} vs {c['loss']:.6f}")
    assert abs(float(loss) - c["loss"]) < 1e-4 * max(1.0, abs(c["loss"]))
    loss.backward()
    floor = 1e-3 * max(float(g.abs().max()) for g in c["grads"].values())
    worst = ("", 0.0)
    for name in m._names:
        g_ref, g = c["grads"][name], m.P(name).grad
        assert bool(torch.isfinite(g).all()), name
        e = float((g.cpu() - g_ref).abs().max()) / max(float(g_ref.abs().max()), floor)
        worst = max(worst, (name, e), key=lambda t: t[1])
        assert e < 5e-4, (name, e)
    for i in range(NL):  # q and k take part now (k_proj.bias: its true gradient is zero, only rounding noise)
        for n in ("q_proj.weight", "q_proj.bias", "k_proj.weight"):
            assert float(m.P(f"layers.{i}.encoder_attn.{n}").grad.abs().max()) > 0.0, (i, n)
    assert tuple(enc_d.grad.shape) == tuple(c["enc"].shape)
    e = float((enc_d.grad.cpu() - c["denc"]).abs().max()) / float(c["denc"].abs().max())
    print(f"PARITY txdec_cross d{d} S{s} worst gradient {worst[0]} err={worst[1]:.3e}, d(enc) err={e:.3e}")
    assert e < 5e-4, e


def test_one_encoder_position_keeps_the_constant_path_bit_for_bit(dev):
    """enc [1, R, d], with a mask too: the logits and every gradient of the 2-D call, bit for bit (the atomically
    accumulated embedding-table gradient within its documented run-to-run bound)."""
    from vidsitu_amd.flat_module import FlatTrainFn
    from vidsitu_amd.hf_gpt2_fseq import lm_loss

    d, heads = 64, 4
    w = txdec_ref.make_weights(VOC, d, FFN, NL, OUT, PAD, seed=3)
    m = _model(dev, w, d, heads)
    toks = _tokens(seed=2).to(dev)
    enc = torch.randn(1, ROWS, d, generator=torch.Generator().manual_seed(1)).to(dev)
    mask = torch.zeros(ROWS, 1, dtype=torch.bool, device=dev)
    mask[2] = True  # one key: the mask cannot matter
    m.eval()
    base = m.forward_logits(toks, enc[0].contiguous())
    assert torch.equal(base, m.forward_logits(toks, enc)) and torch.equal(base, m.forward_logits(toks, enc, mask))
    m.train()

    def run(*inputs):
        tick = torch.zeros(1, device=dev, requires_grad=True)
        lm_loss(FlatTrainFn.apply(m, toks, *inputs, tick), toks, PAD).backward()
        return {n: m.P(n).grad.clone() for n in m._names}, inputs[0].grad

    e2 = enc[0].clone().requires_grad_(True)
    g2, de2 = run(e2)
    e3 = enc.clone().requires_grad_(True)
    g3, de3 = run(e3, mask)
    # the embedding table's gradient is accumulated atomically (vs_embed_scatter_bwd): two runs of one call differ
    # in its last bits too (profiles/flat_module.txt: within 1e-5 of the maximum); everything else is bit for bit
    emb = "embed_tokens.weight"
    differ = [n for n in g2 if n != emb and not torch.equal(g2[n], g3[n])]
    assert not differ, differ
    assert float((g2[emb] - g3[emb]).abs().max()) <= 1e-5 * float(g2[emb].abs().max())
    assert tuple(de3.shape) == (1, ROWS, d) and torch.equal(de3[0], de2)
    for i in range(NL):  # one key: no gradient reaches q / k
        assert float(g3[f"layers.{i}.encoder_attn.q_proj.weight"].abs().max()) == 0.0


@pytest.mark.parametrize("d,heads", [(64, 4), (256, 2)], ids=["dh16", "dh128"])
def test_cached_decode_equals_the_whole_sequence_pass(d, heads, dev):
    from vidsitu_amd.hf_gpt2_fseq import KVCacheState

    c = _case(d, heads, 5)
    m = _model(dev, c["w"], d, heads).eval()
    toks = torch.randint(0, VOC - 1, (ROWS, 10), generator=torch.Generator().manual_seed(4)).to(dev)
    enc, mask = c["enc"].to(dev), c["pad_mask"].to(dev)
    full = m.forward_logits(toks, enc, mask)
    st = KVCacheState()
    with torch.no_grad():
        m.begin_incremental(st, m.enc_rows(enc, ROWS, mask), ROWS, 12)
    assert tuple(st.ck.shape) == (NL, ROWS, heads, 5, d // heads) and st.cmask.dtype == torch.uint8
    for t in range(toks.shape[1]):
        step = m.forward_step(toks[:, t].contiguous(), st)
        err = float((step - full[:, t]).abs().max()) / float(full.abs().max())
        assert err < 2e-4, (t, err)


class _Tok:
    pad_token_id, eos_token_id = PAD, ref.EOS

    def __len__(self):
        return VOC

    def pad(self):
        return PAD

    def eos(self):
        return ref.EOS

    def unk(self):
        return ref.EOS


class _EncDec(torch.nn.Module):
    """Minimal `SeqGenCustom` model (the `_OracleDec` pattern of tests/test_gpu_txdec.py): a fixed masked source per
    sentence + the decoder."""

    def __init__(self, dec_model):
        super().__init__()
        from vidsitu_amd.fseq_txdec import TxDecoderReal
        from vidsitu_amd.mdl_sf_base import EncoderOut, Reorderer

        self.use_encoder = True
        dec = TxDecoderReal.__new__(TxDecoderReal)
        torch.nn.Module.__init__(dec)
        dec.model, dec.pad_idx = dec_model, PAD
        self.decoder = dec
        self.enc = self.pad_mask = None
        self._EO, self._re = EncoderOut, Reorderer()

    def max_decoder_positions(self):
        return self.decoder.model.max_positions - 1

    def forward_encoder(self, inp):
        return self._EO(encoder_out=self.enc, encoder_padding_mask=self.pad_mask, encoder_embedding=None,
                        encoder_states=None, src_tokens=None, src_lengths=None)

    def reorder_encoder_out(self, encoder_out, new_order):
        return self._re.reorder_encoder_out(encoder_out, new_order)


@functools.lru_cache(maxsize=None)
def _beam(s):
    return ref.beam_case(s, ref.BEAM_SEEDS[s])


@pytest.mark.parametrize("device_search", [True, False], ids=["device", "host"])
def test_beam_search_tokens_bit_exact_vs_oracle(device_search, dev):
    """A masked S = 5 source, three uses of one shape (eager, capture, replay), then a second generation with
    another source length (S = 3): a new session, still the oracle's tokens.  No sentence is left out."""
    from vidsitu_amd.seq_gen import SeqGenCustom

    c5 = _beam(5)
    m = _model(dev, c5["w"], ref.D, ref.HEADS).eval()
    lm = _EncDec(m)
    sample = {"src_tokens": torch.zeros(ref.BSZ, 1, dtype=torch.long, device=dev),
              "src_lengths": torch.ones(ref.BSZ, dtype=torch.long, device=dev)}
    sessions = set()
    for s, uses in ((5, 3 if device_search else 1), (3, 1)):
        c = _beam(s)
        assert c["gap"] > 1e-4  # the comparison never rests on a tie (asserted on the CPU too)
        lm.enc, lm.pad_mask = c["enc"].to(dev), c["pad_mask"].to(dev)
        for use in range(uses):
            gen = SeqGenCustom([lm], _Tok(), beam_size=ref.BEAM, max_len_b=ref.MAX_LEN_B, min_len=1,
                               device_search=device_search)
            got = gen._generate(sample, prefix_tokens=torch.from_numpy(c["prefix"]).to(dev))
            assert len(got) == ref.BSZ
            for sent in range(ref.BSZ):
                want = c["want"][sent]
                assert [h["tokens"].tolist() for h in got[sent]] == [h["tokens"].tolist() for h in want], (s, use, sent)
                for hg, hw in zip(got[sent], want):
                    assert abs(float(hg["score"]) - hw["score"]) < 1e-4
        if device_search:
            sessions.add(list(lm.decoder._vs_search_sessions)[-1])
    if device_search:
        assert len(sessions) == 2, "another source length opens another session"


class _T:
    pad_token_id = PAD

    def __len__(self):
        return VOC


@pytest.mark.parametrize("l,padded", [(5, False), (20, True)], ids=["small", "masked"])
def test_text_mode_encoder_matches_the_restatement(l, padded, dev, monkeypatch):
    """`TxEncoderOld` on token ids: L = 5 without padding takes the L <= 16 kernels, L = 20 with padding the masked
    matrix-unit kernels; output, every parameter gradient and the embedding gradient."""
    from types import SimpleNamespace
    from vidsitu_amd import ops
    from vidsitu_amd.fseq_txdec import TxEncoderOld

    d, ffn, heads, nl = 128, 256, 8, 2
    cfg = SimpleNamespace(tx_dec=SimpleNamespace(encoder_embed_dim=d, encoder_ffn_embed_dim=ffn,
                                                 encoder_attention_heads=heads, encoder_layers=nl, dropout=0.0))
    enc = TxEncoderOld(cfg, SimpleNamespace(gpt2_hf_tok=_T()), text=True)
    g = torch.Generator().manual_seed(21)
    w = txdec_ref.make_encoder_weights(d, ffn, nl, seed=11)
    emb = torch.randn(VOC, d, generator=g) * d ** -0.5
    emb[PAD] = 0
    enc.load_state_dict(dict(w, **{"embed_tokens.weight": emb}), strict=True)
    enc = enc.to(dev).train()
    src = torch.randint(0, VOC - 1, (3, l), generator=g)
    if padded:
        src[1, l - 7:] = PAD
        src[2, 1:] = PAD
    wg = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    emb_g = emb.clone().requires_grad_(True)
    out_ref = ref.text_encoder_forward(wg, emb_g, src, PAD, heads, nl)
    g_out = torch.randn(out_ref.shape, generator=g)
    if padded:
        g_out = g_out * src.ne(PAD).t().unsqueeze(-1)  # the outputs at padded positions feed nothing downstream
    (out_ref * g_out).sum().backward()
    calls = {"small": 0, "pad": 0}
    small, pad_fn = ops.attn_small_fwd, ops.attn_pad
    monkeypatch.setattr(ops, "attn_small_fwd", lambda *a, **k: (calls.__setitem__("small", calls["small"] + 1),
                                                                small(*a, **k))[1])
    monkeypatch.setattr(ops, "attn_pad", lambda *a, **k: (calls.__setitem__("pad", calls["pad"] + 1),
                                                          pad_fn(*a, **k))[1])
    out = enc(src.to(dev), src_lengths=None, return_all_hiddens=True)
    assert calls == ({"small": 0, "pad": nl} if padded else {"small": nl, "pad": 0}), calls
    assert tuple(out.encoder_out.shape) == (l, 3, d) and len(out.encoder_states) == nl
    assert torch.equal(out.encoder_padding_mask.cpu(), src.eq(PAD))
    valid = src.ne(PAD).t()
    err = float((out.encoder_out.detach().cpu() - out_ref.detach())[valid].abs().max()) / float(out_ref.abs().max())
    print(f"PARITY text encoder L{l} out err={err:.3e}")
    assert err < 2e-4, err
    (out.encoder_out * g_out.to(dev)).sum().backward()
    sd = dict(enc.named_parameters())
    wg["embed_tokens.weight"] = emb_g
    floor = 1e-3 * max(float(v.grad.abs().max()) for v in wg.values())
    for name, r in wg.items():
        e = float((sd[name].grad.cpu() - r.grad).abs().max()) / max(float(r.grad.abs().max()), floor)
        assert e < 5e-4, (name, e)
    assert float(sd["embed_tokens.weight"].grad.abs().max()) > 0.0


@pytest.mark.parametrize("src", ["prompt", "vb"])
def test_txed_only_row_trains_and_generates(src, dev):
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval
    from vidsitu_amd.optim import ArenaAdam, ParamArena
    from vidsitu_amd.seq_gen import SeqGenCustom

    cfg = get_cfg({"task_type": "vb_arg", "mdl.mdl_name": "txed_only", "mdl.tx_dec_type": "txdec",
                   "mdl.tx_enc_type": "old", "mdl.txed_src": src, "tx_dec.decoder_layers": 1,
                   "tx_dec.encoder_layers": 1, "synth.gpt2_vocab": 211, "gen.beam_size": 2, "gen.max_len_b": 6})
    comm = synth_data.make_comm(cfg)
    sel = get_mdl_loss_eval(cfg)
    torch.manual_seed(0)
    mdl = sel["mdl"](cfg=cfg, comm=comm).to(dev).train()
    batch = synth_data.synth_srl_batch(comm, bs=2, n_ev=3, seq_len=10, device=dev)
    opt = ArenaAdam(ParamArena(mdl, adopt_conv=False), lr=3e-4)
    loss_fn = sel["loss"](cfg, comm)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = loss_fn(mdl(batch), batch)["loss"]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"txed_only txed_src={src}: losses {losses}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert mdl.encoder.embed_tokens.weight.grad is not None
    if src == "vb":  # the source sequence reached the cross-attention kernels: q / k of the encoder attention learn
        assert float(mdl.decoder.model.P("layers.0.encoder_attn.q_proj.weight").grad.abs().max()) > 0.0
    mdl.eval()
    gen = SeqGenCustom([mdl], comm.gpt2_hf_tok, beam_size=2, max_len_b=6, min_len=1)
    out = mdl.forward_gen(dict(batch), gen)
    assert out.dim() == 4 and tuple(out.shape[:3]) == (2, 3, 1) and out.shape[3] >= 2


def test_main_dist_trains_and_generates_the_txed_only_row(dev, tmp_path):
    """`python main_dist.py <uid> --task_type=vb_arg --mdl.mdl_name=txed_only ... --mdl.txed_src=vb` in a fresh child
    process, as a user's run is."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    cmd = [sys.executable, "main_dist.py", "t_txed", "--task_type=vb_arg", "--mdl.mdl_name=txed_only",
           "--mdl.tx_dec_type=txdec", "--mdl.tx_enc_type=old", "--mdl.txed_src=vb", "--tx_dec.decoder_layers=1",
           "--tx_dec.encoder_layers=1", "--synth.gpt2_vocab=97", "--train.bs=2", "--ds.vsitu.num_ev=2",
           "--train.lr=1e-3", "--overfit_batch=True", "--gen.beam_size=2", "--gen.max_len_b=8",
           f"--misc.tmp_path={tmp_path}", "--steps=4"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    err = "\n".join(ln for ln in r.stderr.splitlines() if "frame #" not in ln)[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + err
    m = re.search(r"loss ([-\d.e]+) -> ([-\d.e]+)", r.stdout)
    assert m, r.stdout
    first, last = float(m.group(1)), float(m.group(2))
    print(f"main_dist txed_only vb: loss {first:.4f} -> {last:.4f}")
    assert np.isfinite(last) and last < first, r.stdout
