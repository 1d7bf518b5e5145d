"""fairseq's `TransformerDecoder` as `TxDecoderReal` configures it (`vidsitu_code/mdl_sf_base.py:435-446`,
`configs/vsitu_tx_cfgs/transformer.yaml`) on the HIP kernels: post-norm layers
(self attention -> add & norm -> encoder attention -> add & norm -> relu FFN -> add & norm), embed scale
sqrt(d), sinusoidal positions `padding_idx + 1 + t`, `project_out_dim` d -> decoder_output_dim and an
untied `output_projection`, both without bias.  Parameter names / shapes are fairseq's, so its checkpoints
load (`layers.N.self_attn.q_proj.weight`, ...).

* The three self-attention projections run as ONE GEMM on a concatenated [3d, d] weight (cached copy).
* The video rows' encoder output has ONE position per decoder row (`SFPreFeats_TxEncDec.forward_encoder`,
  `mdl_sf_base.py:806-832`: `[1, B*n_ev, 1024]`), so the softmax over encoder positions is exactly 1 and
  encoder attention is `out_proj(v_proj(enc))` broadcast over the target positions -- a per-row constant
  (its q / k projections get exactly zero gradient, as autograd gives them).
* A source of S > 1 positions (`[S, R, d]`, the `txed_only` row's text encoder) is attended over by the
  cross-attention kernels (csrc/attn_cross.hip): q_proj GEMM of the decoder rows, ONE k | v GEMM of the encoder rows on
  a concatenated [2d, d] weight, `ops.attn_cross`, out_proj.  `encoder_padding_mask` (True = padding) masks keys, with
  weight exactly 0.  A source whose positions are ALL padding runs unmasked -- the one rule every padding-masked
  kernel here shares; fairseq's softmax gives NaN there.  The kernels hold K and V of a head in LDS: at d 1024 / 8 heads
  S <= 112 forward and S <= 96 backward; a longer source is refused.
* Training: one autograd node (`flat_module.FlatTrainFn`; `TransformerDecoderHip` is a `FlatParamModule`, which
  owns registration, state dict and the cached copies) -- forward keeps the activations, a hand-written backward
  writes every parameter gradient (overwrite semantics) and returns the gradient of the encoder output.  Dropout
  (`dropout` after the embedding and after each sub-layer; attention / activation dropout are 0 in the
  reference's YAML) through mask operands of the fused add + layernorm kernel.
* Generation: a KV cache per layer read through the beam ancestry table (`vs_attn_decode`), the encoder
  attention constant computed once per generation (`begin_incremental`), so decode steps never read the
  encoder output and can be captured in hipGraphs (`seq_gen._DeviceSearchSession`).
"""
import math
from collections import namedtuple

import torch
from torch import nn

from . import ops
from .flat_module import FlatParamModule, FlatTrainFn
from .transformer_code import AddLayerNormFn, AttnSmallFn, LinearFn, hip_linear


# An encoder output of S > 1 positions as the kernels take it: rows f32 [R*S, d] (row-major over (r, s)), mask u8
# [R, S] (1 = valid) or None
EncSeq = namedtuple("EncSeq", "rows mask s")


def _xavier(out_f, in_f, gain=1.0):
    t = torch.empty(out_f, in_f)
    nn.init.xavier_uniform_(t, gain=gain)
    return t


class TransformerDecoderHip(FlatParamModule):
    _CACHES = ("_cat",  # layer -> concatenated q | k | v projection of the self attention
               "_ccat")  # layer -> concatenated k | v projection of the encoder attention
    _CAPTURE_MSG = "decoder weight copies must exist before a graph capture (run one eager step)"

    def __init__(self, vocab, d_model, ffn, n_head, n_layer, out_dim, pad, dropout=0.1, max_positions=1024):
        super().__init__()
        self.vocab, self.d_model, self.ffn, self.n_head, self.n_layer = vocab, d_model, ffn, n_head, n_layer
        self.out_dim, self.pad, self.p_drop, self.max_positions = out_dim, pad, float(dropout), max_positions
        p = {}
        emb = torch.randn(vocab, d_model) * d_model ** -0.5
        emb[pad] = 0
        p["embed_tokens.weight"] = emb
        for i in range(n_layer):
            q = f"layers.{i}."
            for att in ("self_attn", "encoder_attn"):
                for pr in ("k_proj", "v_proj", "q_proj", "out_proj"):  # MultiheadAttention.reset_parameters
                    p[q + f"{att}.{pr}.weight"] = _xavier(d_model, d_model,
                                                          1.0 if pr == "out_proj" else 1 / math.sqrt(2))
                    p[q + f"{att}.{pr}.bias"] = torch.zeros(d_model)
                p[q + f"{att}_layer_norm.weight"] = torch.ones(d_model)
                p[q + f"{att}_layer_norm.bias"] = torch.zeros(d_model)
            p[q + "fc1.weight"], p[q + "fc1.bias"] = _xavier(ffn, d_model), torch.zeros(ffn)
            p[q + "fc2.weight"], p[q + "fc2.bias"] = _xavier(d_model, ffn), torch.zeros(d_model)
            p[q + "final_layer_norm.weight"] = torch.ones(d_model)
            p[q + "final_layer_norm.bias"] = torch.zeros(d_model)
        p["project_out_dim.weight"] = _xavier(out_dim, d_model)
        p["output_projection.weight"] = torch.randn(vocab, out_dim) * out_dim ** -0.5
        self._register_flat(p)
        self._tab = {}  # device -> position table (derived from no parameter: survives `_drop_copies`)

    # ---- fairseq-compatible state dict -------------------------------------------------------------
    def _extra_state(self, prefix, keep_vars):
        dev = self.P("embed_tokens.weight").device
        return {prefix + "embed_positions._float_tensor": torch.zeros(1, device=dev),
                prefix + "version": torch.tensor([3.0], device=dev)}

    def _tolerated_on_load(self, key):
        return key in ("embed_positions._float_tensor", "version")

    def _qkv(self, i):
        """Concatenated self-attention projection [3d, d] / [3d] of layer i (q | k | v)."""
        q = f"layers.{i}.self_attn."
        return self._copy(self._cat, i, self.P(q + "q_proj.weight"), lambda: (
            torch.cat([self.P(q + f"{n}_proj.weight").detach() for n in "qkv"]).contiguous(),
            torch.cat([self.P(q + f"{n}_proj.bias").detach() for n in "qkv"]).contiguous()))

    def _ckv(self, i):
        """Concatenated encoder-attention projection [2d, d] / [2d] of layer i (k | v)."""
        q = f"layers.{i}.encoder_attn."
        return self._copy(self._ccat, i, self.P(q + "k_proj.weight"), lambda: (
            torch.cat([self.P(q + f"{n}_proj.weight").detach() for n in "kv"]).contiguous(),
            torch.cat([self.P(q + f"{n}_proj.bias").detach() for n in "kv"]).contiguous()))

    def _pos_table(self, device):
        """Row 0 = zeros (padding); row 1 + t = the sinusoid of position padding_idx + 1 + t."""
        return self._copy(self._tab, str(device), self.P("embed_tokens.weight"),
                          lambda: sinusoid_table(self.pad, self.max_positions, self.d_model, device))

    def _embed(self, tokens, pos0=None):
        """tokens i64 [R, L] -> f32 [R*L, d]; pos0: every token sits at target position pos0 (one
        incremental step, fairseq's `positions[:, -1:]`), else `utils.make_positions`."""
        if pos0 is None:
            mask = tokens.ne(self.pad)
            idx = torch.cumsum(mask, dim=1) * mask
        else:
            idx = torch.full_like(tokens, pos0 + 1)
        return ops.embed_pos_fwd(tokens, self.P("embed_tokens.weight"), self._pos_table(tokens.device), idx,
                                 math.sqrt(self.d_model))

    def _cross_const(self, i, enc2d):
        """Encoder attention over ONE encoder position: out_proj(v_proj(enc)) per row -> ([R, d], cv)."""
        q = f"layers.{i}.encoder_attn."
        cv = ops.gemm_nt(enc2d, self.P(q + "v_proj.weight"), self.P(q + "v_proj.bias"))
        return ops.gemm_nt(cv, self.P(q + "out_proj.weight"), self.P(q + "out_proj.bias")), cv

    @staticmethod
    def enc_rows(encoder_out, rows, pad_mask=None):
        """EncoderOut / tensor [S, R, d] (+ its padding mask, bool [R, S], True = padding) -> None, [R, d] for S = 1
        (one key: the mask cannot matter, the constant path) or an `EncSeq` for S > 1.  No host sync."""
        if encoder_out is None:
            return None
        enc = encoder_out.encoder_out if hasattr(encoder_out, "encoder_out") else encoder_out
        if pad_mask is None:
            pad_mask = getattr(encoder_out, "encoder_padding_mask", None)
        if enc.dim() != 3 or enc.shape[1] != rows:
            raise ops._lib.VsError(f"encoder output {tuple(enc.shape)}: [S, {rows}, d] expected")
        s = enc.shape[0]
        if s == 1:
            return enc[0].float().contiguous()
        mask = None
        if pad_mask is not None:
            if tuple(pad_mask.shape) != (rows, s):
                raise ops._lib.VsError(f"encoder_padding_mask {tuple(pad_mask.shape)}: [{rows}, {s}] expected")
            mask = pad_mask.logical_not().to(torch.uint8).contiguous()
        return EncSeq(enc.float().transpose(0, 1).reshape(rows * s, enc.shape[2]), mask, s)

    def _cross_seq(self, i, x1, seq, r, l):
        """Encoder attention over S > 1 positions -> (sub-layer output [R*L, d], cq, ckv, co)."""
        q = f"layers.{i}.encoder_attn."
        wkv, bkv = self._ckv(i)
        cq = ops.gemm_nt(x1, self.P(q + "q_proj.weight"), self.P(q + "q_proj.bias"))
        ckv = ops.gemm_nt(seq.rows, wkv, bkv)
        co = ops.attn_cross(cq, ckv, seq.mask, r, l, seq.s, self.n_head)
        return ops.gemm_nt(co, self.P(q + "out_proj.weight"), self.P(q + "out_proj.bias")), cq, ckv, co

    # ---- whole-sequence pass ------------------------------------------------------------------------
    def _forward_seq(self, tokens, enc, train, enc_mask=None):
        if not tokens.is_cuda:
            raise ops._lib.VsError("the decoder runs on the HIP kernels only (GPU tensor required)")
        r, l = tokens.shape
        d, p = self.d_model, self.p_drop if train else 0.0
        enc3 = enc is not None and not isinstance(enc, EncSeq) and enc.dim() == 3  # d(enc) takes the input's shape
        if enc3:
            enc = self.enc_rows(enc, r, enc_mask)
        seq = enc if isinstance(enc, EncSeq) else None
        enc2d = None if seq is not None else enc
        km = tokens.ne(self.pad).to(torch.uint8).contiguous()

        def mask():
            return ops.dropout_mask((r * l, d), p, tokens.device) if p > 0 else None

        x = self._embed(tokens)
        m0 = mask()
        if m0 is not None:
            x = x * m0
        layers = []
        for i in range(self.n_layer):
            q = f"layers.{i}."
            wqkv, bqkv = self._qkv(i)
            qkv = ops.gemm_nt(x, wqkv, bqkv)
            o = ops.attn_causal(qkv, km, r, l, self.n_head)
            sa = ops.gemm_nt(o, self.P(q + "self_attn.out_proj.weight"), self.P(q + "self_attn.out_proj.bias"))
            m1 = mask()
            x1, mu1, rs1 = ops.add_layernorm_fwd(x, sa, self.P(q + "self_attn_layer_norm.weight"),
                                                 self.P(q + "self_attn_layer_norm.bias"), 1e-5, rmask=m1)
            if seq is not None:
                ca, cq, ckv, co = self._cross_seq(i, x1, seq, r, l)
                cv = (cq, ckv, co)
            elif enc2d is not None:
                co, cv = self._cross_const(i, enc2d)
                ca = co.repeat_interleave(l, dim=0)
            if enc is not None:
                m2 = mask()
                x2, mu2, rs2 = ops.add_layernorm_fwd(x1, ca, self.P(q + "encoder_attn_layer_norm.weight"),
                                                     self.P(q + "encoder_attn_layer_norm.bias"), 1e-5, rmask=m2)
            else:
                cv = ca = m2 = mu2 = rs2 = None
                x2 = x1
            f1 = ops.gemm_nt(x2, self.P(q + "fc1.weight"), self.P(q + "fc1.bias"), act=ops.ACT_RELU)
            f2 = ops.gemm_nt(f1, self.P(q + "fc2.weight"), self.P(q + "fc2.bias"))
            m3 = mask()
            x3, mu3, rs3 = ops.add_layernorm_fwd(x2, f2, self.P(q + "final_layer_norm.weight"),
                                                 self.P(q + "final_layer_norm.bias"), 1e-5, rmask=m3)
            if train:
                layers.append((x, qkv, o, sa, m1, mu1, rs1, x1, cv, ca, m2, mu2, rs2, x2, f1, f2, m3, mu3, rs3))
            x = x3
        po = ops.gemm_nt(x, self.P("project_out_dim.weight"))
        logits = ops.gemm_nt(po, self.P("output_projection.weight"))
        if train:
            self._saved = (tokens, km, r, l, enc2d, m0, layers, x, po, seq, enc3)
        return logits.view(r, l, -1)

    @torch.no_grad()
    def forward_logits(self, tokens, enc=None, enc_mask=None):
        """tokens i64 [R, L]; enc f32 [R, d] (one encoder position per row), [S, R, d] with enc_mask bool [R, S]
        (True = padding) or None, or None -> logits f32 [R, L, V] (no dropout)."""
        return self._forward_seq(tokens, enc, False, enc_mask)

    def forward_train(self, tokens, enc=None, enc_mask=None):
        return self._forward_seq(tokens, enc, True, enc_mask)

    # ---- backward ------------------------------------------------------------------------------------
    @torch.no_grad()
    def backward(self, dlogits):
        """dlogits [R*L, V] -> every parameter's .grad (overwritten); returns the gradient of the encoder output in
        the shape it came in ([R, d], [S, R, d]) or None."""
        tokens, km, r, l, enc2d, m0, layers, x_last, po, seq, enc3 = self._saved
        self._saved = None
        d = self.d_model
        dlogits = dlogits.reshape(r * l, -1)
        dpo = self._linear_bwd("output_projection", po, dlogits, bias=False)
        dx = self._linear_bwd("project_out_dim", x_last, dpo, bias=False)
        denc = None
        for i in reversed(range(self.n_layer)):
            q = f"layers.{i}."
            x, qkv, o, sa, m1, mu1, rs1, x1, cv, ca, m2, mu2, rs2, x2, f1, f2, m3, mu3, rs3 = layers[i]
            dx2_a, df2, _, _ = ops.add_layernorm_bwd(dx, x2, f2, self.P(q + "final_layer_norm.weight"), mu3, rs3,
                                                     rmask=m3, dg_out=self._grad(q + "final_layer_norm.weight"),
                                                     db_out=self._grad(q + "final_layer_norm.bias"))
            df1 = ops.relu_bwd(self._linear_bwd(q + "fc2", f1, df2), f1)
            dx2 = ops.add_f32(dx2_a, self._linear_bwd(q + "fc1", x2, df1))
            if seq is not None:
                cq, ckv, co = cv
                dx1_a, dca, _, _ = ops.add_layernorm_bwd(dx2, x1, ca, self.P(q + "encoder_attn_layer_norm.weight"),
                                                         mu2, rs2, rmask=m2,
                                                         dg_out=self._grad(q + "encoder_attn_layer_norm.weight"),
                                                         db_out=self._grad(q + "encoder_attn_layer_norm.bias"))
                dco = self._linear_bwd(q + "encoder_attn.out_proj", co, dca)
                dcq, dckv = ops.attn_cross_bwd(cq, ckv, seq.mask, dco, r, l, seq.s, self.n_head)
                dx1 = ops.add_f32(dx1_a, self._linear_bwd(q + "encoder_attn.q_proj", x1, dcq))
                wkv, _ = self._ckv(i)
                dw = ops.gemm_nt(ops.transpose_f32(dckv), ops.transpose_f32(seq.rows))  # [2d, d]
                db = ops.colsum_f32(dckv)
                for j, n in enumerate("kv"):
                    self._grad(q + f"encoder_attn.{n}_proj.weight").copy_(dw[j * d:(j + 1) * d])
                    self._grad(q + f"encoder_attn.{n}_proj.bias").copy_(db[j * d:(j + 1) * d])
                de = ops.gemm_nt(dckv, ops.transpose_f32(wkv))  # [R*S, d]
                denc = de if denc is None else ops.add_f32(denc, de)
            elif enc2d is not None:
                dx1, dca, _, _ = ops.add_layernorm_bwd(dx2, x1, ca, self.P(q + "encoder_attn_layer_norm.weight"),
                                                       mu2, rs2, rmask=m2,
                                                       dg_out=self._grad(q + "encoder_attn_layer_norm.weight"),
                                                       db_out=self._grad(q + "encoder_attn_layer_norm.bias"))
                dco = dca.view(r, l, d).sum(dim=1)
                dcv = self._linear_bwd(q + "encoder_attn.out_proj", cv, dco)
                de = self._linear_bwd(q + "encoder_attn.v_proj", enc2d, dcv)
                denc = de if denc is None else ops.add_f32(denc, de)
                for pr in ("q_proj", "k_proj"):  # softmax over one key: no gradient reaches q / k
                    self._grad(q + f"encoder_attn.{pr}.weight").zero_()
                    self._grad(q + f"encoder_attn.{pr}.bias").zero_()
            else:
                dx1 = dx2
                for n in self._names:  # unused sub-layer: zero gradients (overwrite semantics)
                    if n.startswith(q + "encoder_attn"):
                        self._grad(n).zero_()
            dx_a, dsa, _, _ = ops.add_layernorm_bwd(dx1, x, sa, self.P(q + "self_attn_layer_norm.weight"), mu1, rs1,
                                                    rmask=m1, dg_out=self._grad(q + "self_attn_layer_norm.weight"),
                                                    db_out=self._grad(q + "self_attn_layer_norm.bias"))
            do = self._linear_bwd(q + "self_attn.out_proj", o, dsa)
            dqkv = ops.attn_causal_bwd(qkv, km, do, r, l, self.n_head)
            wqkv, _ = self._qkv(i)
            dw = ops.gemm_nt(ops.transpose_f32(dqkv), ops.transpose_f32(x))  # [3d, d]
            db = ops.colsum_f32(dqkv)
            for j, n in enumerate("qkv"):
                self._grad(q + f"self_attn.{n}_proj.weight").copy_(dw[j * d:(j + 1) * d])
                self._grad(q + f"self_attn.{n}_proj.bias").copy_(db[j * d:(j + 1) * d])
            dx = ops.add_f32(dx_a, ops.gemm_nt(dqkv, ops.transpose_f32(wqkv)))
        if m0 is not None:
            dx = dx * m0
        demb = self._grad("embed_tokens.weight")
        demb.zero_()
        ops.embed_scatter_bwd(tokens, dx, demb, math.sqrt(d), self.pad)
        self._drop_copies()  # the optimizer is about to change the parameters
        if denc is not None and seq is not None:
            return denc.view(r, seq.s, d).transpose(0, 1).contiguous()
        return denc.unsqueeze(0) if (denc is not None and enc3) else denc

    # ---- incremental decoding --------------------------------------------------------------------------
    def begin_incremental(self, state, enc, rows, max_len):
        """(Re)initialise an incremental state for `rows` hypotheses: caches allocated once, the
        encoder-attention constants of this generation written into static buffers -- the per-row constant for
        one encoder position (enc [R, d]), per-layer encoder K / V caches and the key mask for an `EncSeq`."""
        seq = enc if isinstance(enc, EncSeq) else None
        enc2d = None if seq is not None else enc
        dev = self.P("embed_tokens.weight").device
        dh = self.d_model // self.n_head
        if state.k is None or state.k.shape[1] != rows or state.k.shape[3] != max_len:
            shape = (self.n_layer, rows, self.n_head, max_len, dh)
            state.k = torch.zeros(shape, dtype=torch.float32, device=dev)
            state.v = torch.zeros(shape, dtype=torch.float32, device=dev)
            state.k2 = state.v2 = None
            state.cross = None
            state.ck = state.cv = state.cmask = None
        state.len = 0
        if seq is None:
            state.ck = state.cv = state.cmask = None
        else:
            shape = (self.n_layer, rows, self.n_head, seq.s, dh)
            if getattr(state, "ck", None) is None or tuple(state.ck.shape) != shape:
                state.ck = torch.empty(shape, dtype=torch.float32, device=dev)
                state.cv = torch.empty(shape, dtype=torch.float32, device=dev)
                state.cmask = torch.empty((rows, seq.s), dtype=torch.uint8, device=dev)
            if seq.mask is None:  # one buffer either way: a captured step's arguments do not change
                state.cmask.fill_(1)
            else:
                state.cmask.copy_(seq.mask)
            for i in range(self.n_layer):
                wkv, bkv = self._ckv(i)
                ops.attn_cross_kv_split(ops.gemm_nt(seq.rows, wkv, bkv), state.ck[i], state.cv[i])
        if enc2d is None:
            state.cross = None
        else:
            if getattr(state, "cross", None) is None:
                state.cross = torch.empty((self.n_layer, rows, self.d_model), dtype=torch.float32, device=dev)
            for i in range(self.n_layer):
                state.cross[i].copy_(self._cross_const(i, enc2d)[0])
        state.ready = True

    @torch.no_grad()
    def forward_step(self, last_tokens, state):
        """One cached step: last_tokens i64 [rows] at target position state.len -> logits [rows, V]."""
        rows = last_tokens.shape[0]
        t = state.len
        x = self._embed(last_tokens.view(rows, 1), pos0=t)
        for i in range(self.n_layer):
            q = f"layers.{i}."
            wqkv, bqkv = self._qkv(i)
            qkv = ops.gemm_nt(x, wqkv, bqkv)
            o = ops.attn_decode(qkv, state.k[i][:rows], state.v[i][:rows], None, t, ancestry=state.anc)
            sa = ops.gemm_nt(o, self.P(q + "self_attn.out_proj.weight"), self.P(q + "self_attn.out_proj.bias"))
            x = ops.add_layernorm_fwd(x, sa, self.P(q + "self_attn_layer_norm.weight"),
                                      self.P(q + "self_attn_layer_norm.bias"), 1e-5)[0]
            if getattr(state, "ck", None) is not None:
                cq = ops.gemm_nt(x, self.P(q + "encoder_attn.q_proj.weight"), self.P(q + "encoder_attn.q_proj.bias"))
                co = ops.attn_cross_decode(cq, state.ck[i], state.cv[i], state.cmask)
                ca = ops.gemm_nt(co, self.P(q + "encoder_attn.out_proj.weight"),
                                 self.P(q + "encoder_attn.out_proj.bias"))
                x = ops.add_layernorm_fwd(x, ca, self.P(q + "encoder_attn_layer_norm.weight"),
                                          self.P(q + "encoder_attn_layer_norm.bias"), 1e-5)[0]
            elif state.cross is not None:
                x = ops.add_layernorm_fwd(x, state.cross[i][:rows], self.P(q + "encoder_attn_layer_norm.weight"),
                                          self.P(q + "encoder_attn_layer_norm.bias"), 1e-5)[0]
            f1 = ops.gemm_nt(x, self.P(q + "fc1.weight"), self.P(q + "fc1.bias"), act=ops.ACT_RELU)
            f2 = ops.gemm_nt(f1, self.P(q + "fc2.weight"), self.P(q + "fc2.bias"))
            x = ops.add_layernorm_fwd(x, f2, self.P(q + "final_layer_norm.weight"),
                                      self.P(q + "final_layer_norm.bias"), 1e-5)[0]
        state.len = t + 1
        return ops.gemm_nt(ops.gemm_nt(x, self.P("project_out_dim.weight")), self.P("output_projection.weight"))

    def reorder_state(self, state, new_order):
        """fairseq reorder_incremental_state (physical gather; the device-side search uses the ancestry
        table instead): row r becomes old row new_order[r]."""
        if state.k is None:
            return
        state.reorder(new_order, self.n_layer)
        if getattr(state, "cross", None) is not None:
            state.cross = state.cross.index_select(1, new_order)
        if getattr(state, "ck", None) is not None:  # the encoder caches and the mask follow their rows too
            state.ck, state.cv = state.ck.index_select(1, new_order), state.cv.index_select(1, new_order)
            state.cmask = state.cmask.index_select(0, new_order)


_TxDecTrainFn = FlatTrainFn  # the name tests/test_gpu_txdec.py imports


class TxDecoderReal(nn.Module):
    """`TxDecoderReal(TransformerDecoder)` (`mdl_sf_base.py:435-446`) with fairseq's decoder call surface:
    `forward(prev_output_tokens, encoder_out=, incremental_state=) -> (logits,)`,
    `reorder_incremental_state`, `max_positions`."""

    uses_encoder_out = False  # decode steps read the constants `begin_incremental` stored in the state

    def __init__(self, cfg, comm):
        super().__init__()
        self.full_cfg, self.comm = cfg, comm
        tok = comm.gpt2_hf_tok
        a = cfg.tx_dec
        self.pad_idx = tok.pad_token_id
        self.model = TransformerDecoderHip(len(tok), a.decoder_embed_dim, a.decoder_ffn_embed_dim,
                                           a.decoder_attention_heads, a.decoder_layers, a.decoder_output_dim,
                                           self.pad_idx, dropout=a.dropout)

    def begin_incremental(self, state, encoder_out, rows, max_len):
        self.model.begin_incremental(state, self.model.enc_rows(encoder_out, rows), rows, max_len)

    def forward(self, prev_output_tokens, src_lengths=None, incremental_state=None, encoder_out=None):
        m = self.model
        if incremental_state:  # KVCacheState is truthy; fairseq's dict-based incremental decoding
            st = incremental_state
            if not getattr(st, "ready", False):
                self.begin_incremental(st, encoder_out, prev_output_tokens.size(0),
                                       getattr(st, "max_len", None) or m.max_positions)
            if st.len != prev_output_tokens.size(1) - 1:
                raise ops._lib.VsError("incremental state out of step with prev_output_tokens")
            return (m.forward_step(prev_output_tokens[:, -1].contiguous(), st).unsqueeze(1),)
        train = self.training and torch.is_grad_enabled()
        enc = None if encoder_out is None else getattr(encoder_out, "encoder_out", encoder_out)
        if enc is not None and enc.dim() == 3 and enc.shape[0] > 1:  # a source sequence: the node takes it whole
            pad_mask = getattr(encoder_out, "encoder_padding_mask", None)
            if train:
                tick = torch.zeros(1, device=prev_output_tokens.device, requires_grad=True)
                return (FlatTrainFn.apply(m, prev_output_tokens, enc.float(), pad_mask, tick),)
            return (m.forward_logits(prev_output_tokens, enc.float(), pad_mask),)
        enc2d = m.enc_rows(encoder_out, prev_output_tokens.size(0))
        if train:
            tick = torch.zeros(1, device=prev_output_tokens.device, requires_grad=True)
            return (FlatTrainFn.apply(m, prev_output_tokens, enc2d, tick),)
        return (m.forward_logits(prev_output_tokens, enc2d),)

    def reorder_incremental_state(self, incremental_state, new_order):
        if incremental_state:
            self.model.reorder_state(incremental_state, new_order)

    def max_positions(self):
        return self.model.max_positions

    def max_decoder_positions(self):
        return self.model.max_positions


# ================================================================================================
# fairseq TransformerEncoder as `TxEncoderOld` uses it (`vidsitu_code/mdl_sf_base.py:246-338`,
# `tx_enc_type: old`): the per-event video features ARE the token embeddings; `src_tokens` (their first
# channel, a float tensor) only drives the position / padding rules.  Post-norm layers, no final norm.
# Built from the autograd functions of the TxEncoderNew path (fused linear, L <= 16 attention, fused
# residual + dropout + layernorm), so the backward is theirs.
# Text mode (`token_embeddings=None`, the `txed_only` row): `embed_tokens(src_tokens)` is looked up (and trained), the
# padding mask reaches the layers; a sequence with padding or past 16 positions attends through the padding-masked
# matrix-unit kernels (`ops.attn_pad`, key-tiled past their LDS limit) on one fused q | k | v GEMM.
# ================================================================================================
class _EmbedPosFn(torch.autograd.Function):
    """scale * emb[tokens] + table[idx] (vs_embed_pos_fwd); the embedding's gradient by vs_embed_scatter_bwd."""

    @staticmethod
    def forward(ctx, emb, tokens, table, idx, scale, pad):
        ctx.save_for_backward(tokens)
        ctx.scale, ctx.pad, ctx.shape = scale, pad, emb.shape
        return ops.embed_pos_fwd(tokens, emb, table, idx, scale)

    @staticmethod
    def backward(ctx, dx):
        (tokens,) = ctx.saved_tensors
        demb = torch.zeros(ctx.shape, dtype=torch.float32, device=dx.device)
        ops.embed_scatter_bwd(tokens, dx.contiguous(), demb, ctx.scale, ctx.pad)
        return demb, None, None, None, None, None


class _AttnPadFn(torch.autograd.Function):
    """Padding-masked self-attention on the fused projection output qkv [R*L, 3D] (ops.attn_pad / attn_pad_bwd)."""

    @staticmethod
    def forward(ctx, qkv, key_mask, r, l, heads):
        ctx.save_for_backward(qkv, key_mask)
        ctx.dims = (r, l, heads)
        return ops.attn_pad(qkv, key_mask, r, l, heads)

    @staticmethod
    def backward(ctx, do):
        qkv, key_mask = ctx.saved_tensors
        return ops.attn_pad_bwd(qkv, key_mask, do.contiguous(), *ctx.dims), None, None, None, None


def sinusoid_table(pad, n_rows, d, device):
    """Row 0 = zeros; row 1 + t = fairseq's sinusoidal embedding of position pad + 1 + t (CPU fp32 math)."""
    half = d // 2
    freq = torch.exp(torch.arange(half, dtype=torch.float) * -(math.log(10000) / (half - 1)))
    ang = torch.arange(pad + 1, pad + 1 + n_rows, dtype=torch.float).unsqueeze(1) * freq.unsqueeze(0)
    tab = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
    if d % 2 == 1:
        tab = torch.cat([tab, torch.zeros(n_rows, 1)], dim=1)
    return torch.cat([torch.zeros(1, d), tab]).contiguous().to(device)


class _FseqSelfAttn(nn.Module):
    def __init__(self, d, heads):
        super().__init__()
        self.k_proj, self.v_proj = nn.Linear(d, d), nn.Linear(d, d)
        self.q_proj, self.out_proj = nn.Linear(d, d), nn.Linear(d, d)
        for m in (self.k_proj, self.v_proj, self.q_proj):
            nn.init.xavier_uniform_(m.weight, gain=1 / math.sqrt(2))
        nn.init.xavier_uniform_(self.out_proj.weight)
        nn.init.zeros_(self.out_proj.bias)
        self.heads, self.scale = heads, math.sqrt(d // heads)

    def forward(self, x, key_mask=None):
        """x [B, L, d]; key_mask u8 [B, L] (1 = valid) or None."""
        b, l, d = x.shape
        if key_mask is None and l <= 16:
            o = AttnSmallFn.apply(hip_linear(self.q_proj, x), hip_linear(self.k_proj, x), hip_linear(self.v_proj, x),
                                  self.heads, self.scale, None)
            return hip_linear(self.out_proj, o)
        projs = (self.q_proj, self.k_proj, self.v_proj)
        qkv = LinearFn.apply(x.reshape(b * l, d), torch.cat([m.weight for m in projs]),
                             torch.cat([m.bias for m in projs]), False, None)
        o = _AttnPadFn.apply(qkv, key_mask, b, l, self.heads)
        return hip_linear(self.out_proj, o).view(b, l, d)


class _FseqEncoderLayer(nn.Module):
    def __init__(self, d, ffn, heads, dropout):
        super().__init__()
        self.self_attn = _FseqSelfAttn(d, heads)
        self.self_attn_layer_norm = nn.LayerNorm(d)
        self.fc1, self.fc2 = nn.Linear(d, ffn), nn.Linear(ffn, d)
        self.final_layer_norm = nn.LayerNorm(d)
        self.p = float(dropout)

    def _mask(self, x):
        if self.training and self.p > 0:
            return ops.dropout_mask((x.numel() // x.shape[-1], x.shape[-1]), self.p, x.device)
        return None

    def forward(self, x, key_mask=None):
        a = self.self_attn(x, key_mask)
        ln = self.self_attn_layer_norm
        x = AddLayerNormFn.apply(x, a, ln.weight, ln.bias, ln.eps, self._mask(a), None)
        f = hip_linear(self.fc2, hip_linear(self.fc1, x, relu=True))
        ln = self.final_layer_norm
        return AddLayerNormFn.apply(x, f, ln.weight, ln.bias, ln.eps, self._mask(f), None)


class TxEncoderOld(nn.Module):
    _want_embedding = False  # text mode: also return scale * embed_tokens(src_tokens) (TxEncoderNew_Conc reads it)

    def _table(self, l, d, device):
        tab = self._tab.get(str(device))
        if tab is None or tab.shape[0] < l + 1:
            tab = self._tab[str(device)] = sinusoid_table(self.padding_idx, max(l, 16), d, device)
        return tab

    def _forward_text(self, src_tokens, return_all_hiddens):
        """src_tokens i64 [B, L]: fairseq's TransformerEncoder on its own embedding table."""
        if src_tokens is None or src_tokens.dtype != torch.int64 or src_tokens.dim() != 2:
            raise ops._lib.VsError("a text encoder takes int64 src_tokens [B, L] (or token_embeddings)")
        if not src_tokens.is_cuda:
            raise ops._lib.VsError("the encoder runs on the HIP kernels only (GPU tensor required)")
        src_tokens = src_tokens.contiguous()
        b, l = src_tokens.shape
        w = self.embed_tokens.weight
        d = w.shape[1]
        valid = src_tokens.ne(self.padding_idx)
        idx = torch.cumsum(valid, dim=1) * valid  # utils.make_positions, as a row of the table
        tab = self._table(l, d, w.device)
        x = _EmbedPosFn.apply(w, src_tokens, tab, idx, self.embed_scale, self.padding_idx).view(b, l, d)
        embed = None
        if self._want_embedding:  # row 0 of the table is zero: the same kernel without the positions
            embed = _EmbedPosFn.apply(w, src_tokens, tab, torch.zeros_like(idx), self.embed_scale,
                                      self.padding_idx).view(b, l, d)
        if self.training and self.p > 0:
            x = x * ops.dropout_mask((b, l, d), self.p, x.device)
        # which attention kernel a layer takes is a host decision: one read of the mask per encoder pass (the encoder
        # runs once per step / generation and is never captured)
        key_mask = None if bool(valid.all()) else valid.to(torch.uint8).contiguous()
        states = [] if return_all_hiddens else None
        for layer in self.layers:
            x = layer(x, key_mask)
            if states is not None:
                states.append(x.transpose(0, 1))
        return self._EncoderOut(encoder_out=x.transpose(0, 1).contiguous(), encoder_padding_mask=~valid,
                                encoder_embedding=embed, encoder_states=states, src_tokens=None, src_lengths=None)

    def __init__(self, cfg, comm, text=False):
        super().__init__()
        from .mdl_sf_base import EncoderOut

        self._EncoderOut = EncoderOut
        self.full_cfg, self.comm = cfg, comm
        tok = comm.gpt2_hf_tok  # comm[comm.dct_id]; the vb_arg task's dictionary (dat_loader.py:61)
        a = cfg.tx_dec
        d = a.encoder_embed_dim
        self.padding_idx = tok.pad_token_id
        # constructed by the reference and part of its checkpoints; used (and trained) only by a text encoder
        # (`text=True`, `forward` without token_embeddings) -- the video rows give the embeddings
        self.embed_tokens = nn.Embedding(len(tok), d, self.padding_idx)
        self.embed_tokens.weight.requires_grad_(bool(text))
        self.embed_scale = math.sqrt(d)
        self.p = float(a.dropout)
        self.layers = nn.ModuleList([_FseqEncoderLayer(d, a.encoder_ffn_embed_dim, a.encoder_attention_heads,
                                                       a.dropout) for _ in range(a.encoder_layers)])
        self._tab = {}

    def forward(self, src_tokens=None, src_lengths=None, return_all_hiddens=False, token_embeddings=None):
        if token_embeddings is None:
            return self._forward_text(src_tokens, return_all_hiddens)
        x = token_embeddings.float()
        if not x.is_cuda:
            raise ops._lib.VsError("the encoder runs on the HIP kernels only (GPU tensor required)")
        b, l, d = x.shape
        tab = self._table(l, d, x.device)
        mask = src_tokens.ne(self.padding_idx)
        idx = torch.cumsum(mask, dim=1) * mask  # utils.make_positions, as a row of the table
        embed = self.embed_scale * x
        x = embed + tab[idx]
        if self.training and self.p > 0:
            x = x * ops.dropout_mask((b, l, d), self.p, x.device)
        states = [] if return_all_hiddens else None
        for layer in self.layers:
            x = layer(x)
            if states is not None:
                states.append(x.transpose(0, 1))
        return self._EncoderOut(encoder_out=x.transpose(0, 1).contiguous(),
                                encoder_padding_mask=src_tokens.eq(self.padding_idx), encoder_embedding=embed,
                                encoder_states=states, src_tokens=None, src_lengths=None)
