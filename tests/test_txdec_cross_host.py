"""Encoder attention over source sequences and the `txed_only` row, without a GPU: the restatement the GPU tests are
held to (tests/txdec_cross_ref.py) against an independent implementation, the selector row and its config key, the
fairseq state-dict names, the C ABI of the new kernels and their LDS limits, and the rank gaps of the beam-search case."""
import math
import os
import re

import pytest
import torch

import txdec_cross_ref as ref
from oracle import txdec_ref
from vidsitu_amd import _lib, synth_data
from vidsitu_amd.extended_config import get_cfg
from vidsitu_amd.mdl_selector import get_mdl_loss_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_torch_nn_transformer_decoder_layer_with_a_memory_mask():
    torch.manual_seed(0)
    vocab, d, ffn, n_layer, out_dim, pad, heads = 50, 32, 48, 2, 16, 49, 4
    w = txdec_ref.make_weights(vocab, d, ffn, n_layer, out_dim, pad, seed=3)
    toks = torch.randint(0, vocab - 1, (3, 7))
    toks[0, 5:] = pad
    enc = torch.randn(6, 3, d)
    enc_pad = torch.tensor([[0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 1, 1], [0, 1, 1, 1, 1, 1]], dtype=torch.bool)
    logits = ref.decoder_forward(w, toks, enc, enc_pad, pad, heads, n_layer)
    pos = txdec_ref.make_positions(toks, pad)
    x = math.sqrt(d) * w["embed_tokens.weight"][toks] + txdec_ref.sinusoidal_rows(pos, d) * pos.ne(pad).unsqueeze(-1)
    for i in range(n_layer):
        q = f"layers.{i}."
        layer = torch.nn.TransformerDecoderLayer(d, heads, ffn, dropout=0.0, activation="relu", batch_first=True,
                                                 norm_first=False).eval()
        with torch.no_grad():
            for att, mod in (("self_attn", layer.self_attn), ("encoder_attn", layer.multihead_attn)):
                mod.in_proj_weight.copy_(torch.cat([w[q + f"{att}.{p}_proj.weight"] for p in "qkv"]))
                mod.in_proj_bias.copy_(torch.cat([w[q + f"{att}.{p}_proj.bias"] for p in "qkv"]))
                mod.out_proj.weight.copy_(w[q + f"{att}.out_proj.weight"])
                mod.out_proj.bias.copy_(w[q + f"{att}.out_proj.bias"])
            for mine, theirs in (("self_attn_layer_norm", layer.norm1), ("encoder_attn_layer_norm", layer.norm2),
                                 ("final_layer_norm", layer.norm3)):
                theirs.weight.copy_(w[q + mine + ".weight"])
                theirs.bias.copy_(w[q + mine + ".bias"])
            layer.linear1.weight.copy_(w[q + "fc1.weight"])
            layer.linear1.bias.copy_(w[q + "fc1.bias"])
            layer.linear2.weight.copy_(w[q + "fc2.weight"])
            layer.linear2.bias.copy_(w[q + "fc2.bias"])
            causal = torch.triu(torch.full((7, 7), float("-inf")), 1)
            x = layer(x, enc.transpose(0, 1), tgt_mask=causal, tgt_key_padding_mask=toks.eq(pad),
                      memory_key_padding_mask=enc_pad)
    want = (x @ w["project_out_dim.weight"].t()) @ w["output_projection.weight"].t()
    valid = toks.ne(pad)
    assert float((logits - want)[valid].abs().max()) < 2e-4 * float(want.abs().max())
    # the mask matters, and the restatement runs in fp64 as the kernel tests need it
    assert float((logits - ref.decoder_forward(w, toks, enc, None, pad, heads, n_layer))[valid].abs().max()) > 1e-3
    w64 = {k: v.double() for k, v in w.items()}
    l64 = ref.decoder_forward(w64, toks, enc.double(), enc_pad, pad, heads, n_layer)
    assert l64.dtype == torch.float64 and float((l64 - logits)[valid].abs().max()) < 1e-4 * float(want.abs().max())


def test_cross_attention_restatement_and_its_all_padding_rule():
    g = torch.Generator().manual_seed(1)
    r, l, s, h, d = 3, 4, 5, 2, 8
    q, kv = torch.randn(r, l, d, generator=g), torch.randn(r, s, 2 * d, generator=g)
    mask = torch.tensor([[1, 1, 1, 0, 0], [0, 0, 1, 1, 1], [0, 0, 0, 0, 0]])
    out = ref.cross_attention(q, kv, mask, h)
    want = torch.nn.functional.scaled_dot_product_attention(
        q.view(r, l, h, 4).transpose(1, 2), kv[..., :d].reshape(r, s, h, 4).transpose(1, 2),
        kv[..., d:].reshape(r, s, h, 4).transpose(1, 2),
        attn_mask=ref.valid_keys(mask)[:, None, None, :]).transpose(1, 2).reshape(r, l, d)
    assert float((out - want).abs().max()) < 1e-5
    assert torch.equal(out[2], ref.cross_attention(q, kv, None, h)[2])  # an all-zero row runs unmasked
    assert bool(torch.isfinite(out).all())
    kv2 = kv.clone()
    kv2[0, 3:] += 100.0  # masked keys weigh exactly 0
    assert torch.equal(ref.cross_attention(q, kv2, mask, h)[0], out[0])
    assert ref.cross_attention(q.double(), kv.double(), mask, h).dtype == torch.float64


def test_selector_returns_the_txed_only_row():
    from vidsitu_amd.evl_vsitu import EvalB_Gen
    from vidsitu_amd.mdl_sf_base import LossLambda, Simple_TxDec, Simple_TxEncDec

    sel = get_mdl_loss_eval(get_cfg({"task_type": "vb_arg", "mdl.mdl_name": "txed_only"}))
    assert sel == {"mdl": Simple_TxEncDec, "loss": LossLambda, "evl": EvalB_Gen}
    assert issubclass(Simple_TxEncDec, Simple_TxDec) and hasattr(Simple_TxEncDec, "reorder_encoder_out")


def _small(over=None):
    base = {"task_type": "vb_arg", "mdl.mdl_name": "txed_only", "mdl.tx_dec_type": "txdec", "mdl.tx_enc_type": "old",
            "tx_dec.decoder_layers": 1, "tx_dec.encoder_layers": 2, "synth.gpt2_vocab": 61}
    base.update(over or {})
    cfg = get_cfg(base)
    return cfg, synth_data.make_comm(cfg)


def test_txed_src_key_default_yml_comment_and_refusal():
    assert get_cfg().mdl.txed_src == "prompt"
    yml = open(os.path.join(ROOT, "configs", "vsitu_cfg.yml")).read()
    assert re.search(r"^  txed_src: 'prompt'\s+# addition", yml, re.M)
    from vidsitu_amd.mdl_sf_base import Simple_TxEncDec

    cfg, comm = _small({"mdl.txed_src": "video"})
    with pytest.raises(ValueError, match="txed_src"):
        Simple_TxEncDec(cfg, comm)
    cfg, comm = _small({"mdl.tx_enc_type": "new"})
    with pytest.raises(NotImplementedError, match="given embeddings"):
        Simple_TxEncDec(cfg, comm)
    cfg, comm = _small({"mdl.txed_src": "vb"})
    assert Simple_TxEncDec(cfg, comm).txed_src == "vb"


def test_state_dict_names_are_fairseqs():
    from vidsitu_amd.mdl_sf_base import Simple_TxEncDec

    cfg, comm = _small()
    mdl = Simple_TxEncDec(cfg, comm)
    names = set(mdl.state_dict())
    want = {"encoder.embed_tokens.weight"}
    for i in range(2):
        for p in ("q_proj", "k_proj", "v_proj", "out_proj"):
            want |= {f"encoder.layers.{i}.self_attn.{p}.weight", f"encoder.layers.{i}.self_attn.{p}.bias"}
        for n in ("self_attn_layer_norm", "fc1", "fc2", "final_layer_norm"):
            want |= {f"encoder.layers.{i}.{n}.weight", f"encoder.layers.{i}.{n}.bias"}
    assert want <= names, sorted(want - names)
    enc_names = {n for n in names if n.startswith("encoder.")}
    assert enc_names == want, sorted(enc_names - want)
    dec = {n.split(".", 1)[1] for n in names if n.startswith("decoder.")}
    inner = {n.split(".", 1)[1] if n.startswith("model.") else n for n in dec}
    assert set(txdec_ref.param_names(1)) <= inner
    assert mdl.encoder.embed_tokens.weight.requires_grad and mdl.use_encoder


def test_header_declares_the_cross_attention_symbols():
    hdr = open(os.path.join(ROOT, "include", "vidsitu_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in ("vs_attn_cross_fwd", "vs_attn_cross_bwd", "vs_attn_cross_bwd_scratch_bytes", "vs_attn_cross_fits",
                "vs_attn_cross_decode", "vs_attn_cross_kv_split"):
        assert re.search(rf"\b{sym}\s*\(", hdr), sym
        assert sym in _lib.SIGNATURES


def _lds(s, dh, backward):
    """The documented formulas: K and V of the source at pitch dh + 4, and per wave one (forward) or two
    (backward) strips of 16 score rows at pitch Sp + 4, Sp = S rounded up to 16."""
    sp = (s + 15) // 16 * 16
    return (2 * sp * (dh + 4) + (8 if backward else 4) * 16 * (sp + 4)) * 4


@pytest.mark.parametrize("dh", [16, 32, 64, 128])
def test_cross_fits_agrees_with_the_documented_formulas_at_the_boundary(dh):
    lib = _lib.load()
    limit = 159 * 1024
    for backward in (0, 1):
        fits = [s for s in range(1, 700) if lib.vs_attn_cross_fits(17, s, dh, backward)]
        smax = max(fits)
        assert fits == list(range(1, smax + 1))
        assert _lds(smax, dh, backward) <= limit < _lds(smax + 1, dh, backward)
        assert lib.vs_attn_cross_fits(1, smax, dh, backward) and lib.vs_attn_cross_fits(100000, smax, dh, backward)
    assert max(s for s in range(1, 700) if lib.vs_attn_cross_fits(17, s, 128, 0)) == 112
    assert max(s for s in range(1, 700) if lib.vs_attn_cross_fits(17, s, 128, 1)) == 96
    assert not lib.vs_attn_cross_fits(17, 5, 48, 0) and not lib.vs_attn_cross_fits(0, 5, dh, 0)
    assert not lib.vs_attn_cross_fits(17, 0, dh, 0)
    assert lib.vs_attn_cross_bwd_scratch_bytes(3, 17, 5, 2) == 3 * 2 * 2 * 17 * 16 * 4


def test_refusal_names_the_limit_without_a_gpu():
    lib = _lib.load()
    one = (torch.zeros(4)).data_ptr()
    rc = lib.vs_attn_cross_fwd(one, one, None, one, 1, 17, 113, 1, 128, None)
    assert rc != 0
    msg = lib.vs_last_error_string().decode()
    assert "S = 113" in msg and str(159 * 1024) in msg, msg


@pytest.mark.parametrize("s", sorted(ref.BEAM_SEEDS))
def test_beam_case_never_rests_on_a_tie(s):
    """The oracle's gap between the candidates at ranks 2 * beam and 2 * beam + 1 exceeds 1e-4 at every step of the
    search tests/test_gpu_txdec_cross.py compares token by token, and every sentence finishes with `beam` hypotheses."""
    c = ref.beam_case(s, ref.BEAM_SEEDS[s])
    assert c["gap"] > 1e-4, c["gap"]
    assert all(len(h) == ref.BEAM for h in c["want"])
    assert len({len(c["want"][i][0]["tokens"]) for i in range(ref.BSZ)}) > 1  # hypotheses finish at different steps
    assert bool(c["pad_mask"].any()) and not bool(c["pad_mask"].all(dim=1).any())
