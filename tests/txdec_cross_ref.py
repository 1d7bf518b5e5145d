"""Plain-torch restatement (any dtype, autograd gives the gradients) of what the decoder's encoder attention over a
source of S > 1 positions computes -- the contract of csrc/attn_cross.hip and of `TransformerDecoderHip` with an
`[S, R, d]` encoder output -- and of the text-mode `TxEncoderOld`.  Composed from the pieces of `oracle.txdec_ref`
(fairseq parity is unpinned, as that module says); held against `torch.nn.TransformerDecoderLayer` in
tests/test_txdec_cross_host.py.

The one rule that is the project's and not fairseq's: a source whose positions are ALL padding runs unmasked (the rule
every padding-masked kernel here shares); fairseq's softmax over -inf alone gives NaN there.
"""
import math

import torch
import torch.nn.functional as F

from oracle import txdec_ref as O


def valid_keys(mask):
    """{0,1} [R, S] (1 = valid) -> bool [R, S] of the keys that take part: a row without a valid key keeps them all."""
    v = mask.bool()
    return v | ~v.any(dim=1, keepdim=True)


def cross_attention(q, kv, mask, h):
    """q [R, L, D], kv [R, S, 2D] (k | v), mask {0,1} [R, S] or None -> [R, L, D] (vs_attn_cross_fwd's contract)."""
    r, l, d = q.shape
    s = kv.shape[1]
    dh = d // h
    k, v = kv.split(d, dim=-1)
    q = q.reshape(r, l, h, dh).transpose(1, 2)
    k = k.reshape(r, s, h, dh).transpose(1, 2)
    v = v.reshape(r, s, h, dh).transpose(1, 2)
    a = q @ k.transpose(-1, -2) / math.sqrt(dh)
    if mask is not None:
        a = a.masked_fill(~valid_keys(mask)[:, None, None, :], float("-inf"))
    return (torch.softmax(a, dim=-1) @ v).transpose(1, 2).reshape(r, l, d)


def decoder_forward(w, tokens, enc, enc_pad_mask, pad, n_head, n_layer):
    """tokens i64 [B, L]; enc [S, B, D]; enc_pad_mask bool [B, S] (True = padding) or None -> logits [B, L, V]
    (eval mode).  `oracle.txdec_ref.forward` with `key_padding_mask` handed to the encoder attention."""
    d = w["embed_tokens.weight"].shape[1]
    b, l = tokens.shape
    pos = O.make_positions(tokens, pad)
    pe = (O.sinusoidal_rows(pos, d) * pos.ne(pad).unsqueeze(-1)).to(enc.dtype)
    x = math.sqrt(d) * F.embedding(tokens, w["embed_tokens.weight"]) + pe
    pad_mask = tokens.eq(pad)
    kpm = pad_mask if bool(pad_mask.any()) else None
    causal = torch.triu(torch.full((l, l), float("-inf"), dtype=enc.dtype), 1)
    enc_b = enc.transpose(0, 1)
    ekpm = None if enc_pad_mask is None else ~valid_keys(~enc_pad_mask)
    for i in range(n_layer):
        q = f"layers.{i}."
        x = F.layer_norm(x + _mha(x, x, w, q + "self_attn.", n_head, causal, kpm), (d,),
                         w[q + "self_attn_layer_norm.weight"], w[q + "self_attn_layer_norm.bias"])
        x = F.layer_norm(x + _mha(x, enc_b, w, q + "encoder_attn.", n_head, None, ekpm), (d,),
                         w[q + "encoder_attn_layer_norm.weight"], w[q + "encoder_attn_layer_norm.bias"])
        f = F.linear(F.relu(F.linear(x, w[q + "fc1.weight"], w[q + "fc1.bias"])), w[q + "fc2.weight"],
                     w[q + "fc2.bias"])
        x = F.layer_norm(x + f, (d,), w[q + "final_layer_norm.weight"], w[q + "final_layer_norm.bias"])
    x = F.linear(x, w["project_out_dim.weight"])
    return F.linear(x, w["output_projection.weight"])


def _mha(x_q, x_kv, w, pre, n_head, attn_mask, key_padding_mask):
    """`oracle.txdec_ref._mha` without its cast of the scores to fp32 (the restatement also runs in fp64)."""
    if x_q.dtype == torch.float32:
        return O._mha(x_q, x_kv, w, pre, n_head, attn_mask, key_padding_mask)
    b, l, d = x_q.shape
    s = x_kv.shape[1]
    dh = d // n_head
    q = F.linear(x_q, w[pre + "q_proj.weight"], w[pre + "q_proj.bias"]) * dh ** -0.5
    k = F.linear(x_kv, w[pre + "k_proj.weight"], w[pre + "k_proj.bias"])
    v = F.linear(x_kv, w[pre + "v_proj.weight"], w[pre + "v_proj.bias"])
    q = q.view(b, l, n_head, dh).transpose(1, 2)
    k = k.view(b, s, n_head, dh).transpose(1, 2)
    v = v.view(b, s, n_head, dh).transpose(1, 2)
    a = q @ k.transpose(-1, -2)
    if attn_mask is not None:
        a = a + attn_mask
    if key_padding_mask is not None:
        a = a.masked_fill(key_padding_mask[:, None, None, :], float("-inf"))
    o = (torch.softmax(a, dim=-1) @ v).transpose(1, 2).reshape(b, l, d)
    return F.linear(o, w[pre + "out_proj.weight"], w[pre + "out_proj.bias"])


def text_encoder_forward(w, emb, src_tokens, pad, n_head, n_layer):
    """The text-mode encoder: `oracle.txdec_ref.encoder_forward` fed with the looked-up embeddings
    (emb [V, D], src_tokens i64 [B, L]) -> encoder_out [L, B, D]."""
    return O.encoder_forward(w, F.embedding(src_tokens, emb), src_tokens, pad, n_head, n_layer)


# ---- the beam-search case of tests/test_gpu_txdec_cross.py: the oracle-driven search over a masked source -----------
VOC, D, FFN, NL, OUT, PAD, HEADS = 97, 128, 256, 2, 64, 96, 8
EOS = VOC - 2
BSZ, BEAM, MAX_LEN_B = 4, 3, 9
BEAM_SEEDS = {5: 10, 3: 10}  # source length -> weight seed; test_txdec_cross_host.py asserts their rank gaps


def beam_case(s, seed):
    """-> dict(w, enc [S, BSZ, D], pad_mask bool [BSZ, S], prefix, want, gap): `oracle.beam_ref.generate` driven by
    `decoder_forward` over a right-padded source (lengths S, ..., 1), and the smallest gap the search ever saw between
    the candidates at ranks 2 * beam and 2 * beam + 1 (the last one kept and the first one dropped)."""
    import numpy as np

    from oracle import beam_ref

    w = dict(O.make_weights(VOC, D, FFN, NL, OUT, PAD, seed=seed))
    w["output_projection.weight"] = w["output_projection.weight"].clone()
    w["output_projection.weight"][EOS] *= 2.5  # hypotheses should finish at different steps
    g = torch.Generator().manual_seed(seed + 100 * s)
    enc = torch.randn(s, BSZ, D, generator=g)
    lens = [max(1, s - i * ((s + BSZ - 2) // (BSZ - 1))) for i in range(BSZ)]
    pad_mask = torch.arange(s)[None, :] >= torch.tensor(lens)[:, None]
    prefix = np.array([[5], [9], [5], [70]], dtype=np.int64)

    def step_logits(tokens, sent_ids):
        ids = torch.as_tensor(sent_ids)
        return decoder_forward(w, torch.from_numpy(tokens), enc[:, ids], pad_mask[ids], PAD, HEADS, NL)[:, -1, :].numpy()

    trace = []
    want = beam_ref.generate(step_logits, bsz=BSZ, vocab=VOC, pad=PAD, eos=EOS, unk=EOS, beam_size=BEAM,
                             max_len_b=MAX_LEN_B, min_len=1, prefix_tokens=prefix, max_decoder_positions=63,
                             trace=trace)
    gap = float("inf")
    for t in trace:
        k = 2 * BEAM
        if t.shape[1] > k:
            a, b = t[:, k - 1], t[:, k]
            ok = np.isfinite(a) & np.isfinite(b) & (b > -1e30)
            if ok.any():
                gap = min(gap, float((a - b)[ok].min()))
    return dict(w=w, enc=enc, pad_mask=pad_mask, prefix=prefix, want=want, gap=gap, lens=lens)
