"""Host-side mirror of the reference's GPT-2 decoder wrapper, `HuggingFaceGPT2Decoder`
(`vidsitu_code/hf_gpt2_fseq.py:124-215`), on the HIP kernels of csrc/gpt2_ops.hip.

The reference builds `GPT2LMHeadModel.from_pretrained(cfg.mdl.gpt2_mdl_name)` (huggingface
transformers==3.3.1) and resizes its embeddings to `len(comm.gpt2_hf_tok)`; there is no network
here, so `GPT2LMHeadModelHip` is built from the architecture's dimensions with random weights and
loads a huggingface state dict when one is given (same keys and shapes: `transformer.wte.weight`,
`transformer.h.{i}.attn.c_attn.weight` [in, out] Conv1D layout, ..., `lm_head.weight` tied).
Forward semantics kept: `attention_mask = tokens != pad` (`:185`), default position ids (`:187-193`
stays commented out in the reference), `encoder_out` is accepted and unused exactly as stock GPT-2
(no cross-attention) ignores `encoder_hidden_states` (`:198-204`), returns `(lm_logits,)`.

Incremental decoding: the reference passes empty (falsy) `incremental_state` dicts, so it
re-encodes the whole prefix every step.  The same call with
`incremental_state=None` does that here; given a `KVCacheState` the decoder appends one position to
a KV cache instead -- identical arithmetic, one token of work per step.

Dropout: huggingface's GPT-2 defaults (`embd_pdrop = attn_pdrop = resid_pdrop = 0.1`) are what the reference trains
with (its own overrides at `:144-146` are commented out).  Here the three probabilities are constructor arguments,
0 by default; above 0 the train-mode pass applies the masks of transformers 3.3.1's four dropout sites from the
counter generator of csrc/dropout_rng.h inside the kernels (nothing is stored: the backward regenerates them from the
step's snapshot of the persistent `[seed, step]` device state).  Eval, `forward_logits`, `forward_step` and generation
never apply dropout and never advance the state.

Mixed precision: `matmul="bf16"` (default `"fp32"`) gives the dense projections of the whole-sequence passes --
`forward_train`, `backward`, `forward_logits`: c_attn, attn.c_proj, c_fc, mlp.c_proj and the tied lm_head, forward, dx
and dW -- bf16 operands with fp32 accumulation (`ops.gemm_nt(bf16=True)`: the kernel rounds the fp32 operands as it
loads them, no bf16 copy of a weight or activation exists).  Everything else -- parameters, Adam, layernorm, attention,
gelu, residuals, dropout, the loss, bias and embedding gradients, and the whole cached decode step -- is fp32 in both
modes, so the mode changes no generated token for given weights.

Generation has a switch of its own: `decode_matmul="bf16"` (default `"fp32"`, under which nothing changes bit for bit)
rounds x and W of the five dense projections of `forward_step` to bf16, with fp32 accumulation.  Up to 64 rows (with
d_model % 128 == 0 and a head size of 16, 32 or 64) the step is the packed one on `ops.gemm_nt_packed_bf16`: the weights
are kept as fragment-major bf16 images (`_wpk16`, built once like `_wpk`, which this mode never builds), the
activation images stay fp32 and are rounded by the kernel as it loads them; 1..16 rows take this path too.  Above 64
rows, or at other dimensions, the step runs `_block` / `_head` on `ops.gemm_nt(bf16=True)`.  Embedding, layernorms,
`attn_decode`, the KV cache, gelu and the residuals stay fp32.  The weights are rounded, so this mode MAY change
generated tokens; `forward_logits`, `forward_train`, `backward` and the no-KV-cache path follow `matmul` alone.

`GPT2LMHeadModelHip` is a `flat_module.FlatParamModule`: registration, state dict, the cached weight copies and the
autograd node (`FlatTrainFn`) live there; this file keeps the names / shapes, the arithmetic and `KVCacheState`.
"""
import math

import torch
from torch import nn

from . import ops
from .flat_module import FlatParamModule, FlatTrainFn

GPT2_DIMS = {
    # name: (n_layer, d_model, n_head, n_positions, vocab)
    "gpt2": (12, 768, 12, 1024, 50257),
    "gpt2-medium": (24, 1024, 16, 1024, 50257),
    "gpt2-synth-tiny": (2, 64, 4, 64, 97),  # tests / smoke only
    "gpt2-synth-d128": (2, 128, 4, 64, 97),  # tests only: the smallest model whose decode step takes the packed GEMMs
}


class KVCacheState:
    """Truthy incremental state: per-layer K/V caches [rows, H, Lmax, dh] (double-buffered for the
    beam reorder) and the number of cached positions."""

    def __init__(self):
        self.k = self.v = self.k2 = self.v2 = None
        self.len = 0
        # i32 [rows, Lmax] or None: cache row holding position j of row r (device-side beam search:
        # vs_beam_step permutes this table instead of gathering the cache)
        self.anc = None

    def __bool__(self):
        return True

    def reorder(self, new_order, n_layer):
        """fairseq reorder_incremental_state as a physical gather: row r of the cache becomes old row new_order[r]."""
        if self.k is None:
            return
        if self.anc is not None:
            raise ops._lib.VsError("this cache is reordered through its ancestry table (vs_beam_step)")
        if self.k2 is None:
            self.k2, self.v2 = torch.empty_like(self.k), torch.empty_like(self.v)
        for li in range(n_layer):
            ops.kv_gather(self.k[li], self.k2[li], new_order, self.len)
            ops.kv_gather(self.v[li], self.v2[li], new_order, self.len)
        self.k, self.k2 = self.k2, self.k
        self.v, self.v2 = self.v2, self.v
        self.rows = new_order.numel()


class GPT2LMHeadModelHip(FlatParamModule):
    _CACHES = ("_wt",   # K-contiguous ([out][in]) copies of the Conv1D weights for the kernels
               "_wpk",  # fragment-major copies for the decode-step GEMMs (ops.gemm_nt_packed)
               "_wpk16")  # their bf16 images (ops.gemm_nt_packed_bf16), built instead of `_wpk` by decode_matmul="bf16"
    _CAPTURE_MSG = "GPT-2 weight copies must exist before a graph capture (run one eager step first)"

    _DROP_CAPTURE_MSG = "the GPT-2 dropout state must exist before a graph capture (run one eager step first)"

    def __init__(self, n_layer, d_model, n_head, n_positions, vocab_size, embd_pdrop=0.0, attn_pdrop=0.0,
                 resid_pdrop=0.0, matmul="fp32", decode_matmul="fp32"):
        super().__init__()
        if matmul not in ("fp32", "bf16"):
            raise ValueError(f'matmul must be "fp32" or "bf16", got {matmul!r}')
        if decode_matmul not in ("fp32", "bf16"):
            raise ValueError(f'decode_matmul must be "fp32" or "bf16", got {decode_matmul!r}')
        self.matmul = matmul
        self._bf16 = matmul == "bf16"  # operand precision of the whole-sequence GEMMs (module docstring)
        self.decode_matmul = decode_matmul
        self._bf16_step = decode_matmul == "bf16"  # operand precision of the cached decode step's GEMMs
        self.n_layer, self.d_model, self.n_head, self.n_positions = n_layer, d_model, n_head, n_positions
        self.embd_pdrop, self.attn_pdrop, self.resid_pdrop = float(embd_pdrop), float(attn_pdrop), float(resid_pdrop)
        # (thr, scale) per probability, None at p = 0 (that site then runs today's launches); refuses p outside [0, 1)
        self._drop_embd, self._drop_attn, self._drop_resid = (
            ops.dropout_params(p) if p != 0.0 else None for p in (embd_pdrop, attn_pdrop, resid_pdrop))
        self.config = type("Cfg", (), {"n_positions": n_positions, "n_embd": d_model,
                                       "n_layer": n_layer, "n_head": n_head,
                                       "vocab_size": vocab_size})()
        p = {}

        def add(name, *shape, std=0.02, ones=False):
            t = torch.ones(*shape) if ones else (torch.randn(*shape) * std if std else torch.zeros(*shape))
            p[name] = nn.Parameter(t)

        add("transformer.wte.weight", vocab_size, d_model)
        add("transformer.wpe.weight", n_positions, d_model, std=0.01)
        for i in range(n_layer):
            q = f"transformer.h.{i}."
            for ln in ("ln_1", "ln_2"):
                add(q + ln + ".weight", d_model, ones=True)
                add(q + ln + ".bias", d_model, std=0)
            add(q + "attn.c_attn.weight", d_model, 3 * d_model)
            add(q + "attn.c_attn.bias", 3 * d_model, std=0)
            add(q + "attn.c_proj.weight", d_model, d_model)
            add(q + "attn.c_proj.bias", d_model, std=0)
            add(q + "mlp.c_fc.weight", d_model, 4 * d_model)
            add(q + "mlp.c_fc.bias", 4 * d_model, std=0)
            add(q + "mlp.c_proj.weight", 4 * d_model, d_model)
            add(q + "mlp.c_proj.bias", d_model, std=0)
        add("transformer.ln_f.weight", d_model, ones=True)
        add("transformer.ln_f.bias", d_model, std=0)
        self._register_flat(p)

    # ---- huggingface-compatible state dict -------------------------------------------------
    def _extra_state(self, prefix, keep_vars):
        w = self.P("transformer.wte.weight")
        return {prefix + "lm_head.weight": w if keep_vars else w.detach()}  # tied

    def _tolerated_on_load(self, key):
        # huggingface checkpoints also carry the causal-mask buffers of every block
        return key == "lm_head.weight" or key.endswith((".attn.bias", ".attn.masked_bias"))

    def resize_token_embeddings(self, new_size):
        """transformers PreTrainedModel.resize_token_embeddings: keep the first rows, initialise
        the added ones N(0, 0.02) (the reference adds the SRL / separator tokens, :151-152)."""
        old = self.P("transformer.wte.weight")
        if new_size == old.shape[0]:
            return
        new = torch.randn(new_size, old.shape[1], device=old.device) * 0.02
        n = min(new_size, old.shape[0])
        new[:n] = old.detach()[:n]
        setattr(self, "transformer__wte__weight", nn.Parameter(new))
        self.config.vocab_size = new_size
        self._drop_copies()  # `_wpk` / `_wpk16` may hold a packed copy of the old table

    def _wp(self, name, transposed=True):
        """Fragment-major copy of a weight ([out][in] orientation) for the 17..64-row decode GEMMs."""
        w = self.P(name)
        return self._copy(self._wpk, name, w,
                          lambda: ops.pack_rows_f32(self._w(name) if transposed else w.detach()))

    def _wp16(self, name, transposed=True):
        """Fragment-major bf16 image of a weight ([out][in] orientation) for the bf16-mode decode GEMMs."""
        w = self.P(name)
        return self._copy(self._wpk16, name, w,
                          lambda: ops.pack_rows_bf16(w.detach().t() if transposed else w.detach()))

    def _w(self, name):
        """[out][in] view of a Conv1D weight (transposed once, after load / device move)."""
        w = self.P(name)
        return self._copy(self._wt, name, w, lambda: w.detach().t().contiguous())

    # ---- dropout state -----------------------------------------------------------------------
    def _dropout_on(self):
        return not (self._drop_embd is None and self._drop_attn is None and self._drop_resid is None)

    def _drop_anchor(self):
        return self.P("transformer.wte.weight")

    # ---- compute ---------------------------------------------------------------------------
    def _block(self, i, h, attn_fn, bf16=False):
        q = f"transformer.h.{i}."
        a = ops.add_layernorm_fwd(h, None, self.P(q + "ln_1.weight"), self.P(q + "ln_1.bias"), 1e-5)[0]
        qkv = ops.gemm_nt(a, self._w(q + "attn.c_attn.weight"), self.P(q + "attn.c_attn.bias"), bf16=bf16)
        o = attn_fn(i, qkv)
        h = ops.gemm_nt(o, self._w(q + "attn.c_proj.weight"), self.P(q + "attn.c_proj.bias"), res=h, bf16=bf16)
        m = ops.add_layernorm_fwd(h, None, self.P(q + "ln_2.weight"), self.P(q + "ln_2.bias"), 1e-5)[0]
        f = ops.gemm_nt(m, self._w(q + "mlp.c_fc.weight"), self.P(q + "mlp.c_fc.bias"),
                        act=ops.ACT_GELU_NEW, bf16=bf16)
        return ops.gemm_nt(f, self._w(q + "mlp.c_proj.weight"), self.P(q + "mlp.c_proj.bias"), res=h, bf16=bf16)

    def _head(self, h, bf16=False):
        hf = ops.add_layernorm_fwd(h, None, self.P("transformer.ln_f.weight"),
                                   self.P("transformer.ln_f.bias"), 1e-5)[0]
        return ops.gemm_nt(hf, self.P("transformer.wte.weight"), bf16=bf16)

    @torch.no_grad()
    def forward_logits(self, tokens, attention_mask=None):
        """tokens i64 [R, L] -> logits f32 [R, L, V] (whole-sequence pass)."""
        if not tokens.is_cuda:
            raise ops._lib.VsError("GPT-2 runs on the HIP kernels only (GPU tensor required)")
        r, l = tokens.shape
        km = None if attention_mask is None else attention_mask.to(torch.uint8).contiguous()
        h = ops.gpt2_embed(tokens, self.P("transformer.wte.weight"), self.P("transformer.wpe.weight"))
        for i in range(self.n_layer):
            h = self._block(i, h, lambda _i, qkv: ops.attn_causal(qkv, km, r, l, self.n_head), bf16=self._bf16)
        return self._head(h, bf16=self._bf16).view(r, l, -1)

    @torch.no_grad()
    def forward_step(self, last_tokens, state: KVCacheState, key_mask=None, max_len=None):
        """One cached step: last_tokens i64 [rows] at position state.len -> logits [rows, V]."""
        rows = last_tokens.shape[0]
        dh = self.d_model // self.n_head
        if state.k is None:
            lmax = max_len or self.n_positions
            shape = (self.n_layer, rows, self.n_head, lmax, dh)
            dev = last_tokens.device
            state.k = torch.zeros(shape, dtype=torch.float32, device=dev)
            state.v = torch.zeros(shape, dtype=torch.float32, device=dev)
        t = state.len
        h = ops.gpt2_embed(last_tokens.view(rows, 1), self.P("transformer.wte.weight"),
                           self.P("transformer.wpe.weight"), pos0=t)
        # the packed step: 17..64 rows in fp32 mode (up to 16 rows one wave streams one weight row), 1..64 in bf16 mode
        if ((16 < rows or self._bf16_step) and rows <= 64 and self.d_model % 128 == 0
                and (self.d_model // self.n_head) in (16, 32, 64)):
            return self._forward_step_packed(h, rows, state, key_mask, t)
        for i in range(self.n_layer):
            h = self._block(i, h, lambda li, qkv: ops.attn_decode(qkv, state.k[li][:rows], state.v[li][:rows],
                                                                  key_mask, t, ancestry=state.anc),
                            bf16=self._bf16_step)
        state.len = t + 1
        return self._head(h, bf16=self._bf16_step)

    def _forward_step_packed(self, h, rows, state, key_mask, t):
        """The cached step for 17..64 rows (sentences x beams): every GEMM operand fragment-major --
        weights packed once, activations written in that layout by their producers (layernorm,
        attention, the gelu epilogue) -- so each MFMA fragment load is one contiguous KB.  In bf16 mode
        (1..64 rows) the weights are bf16 images and the kernel rounds the fp32 activation images as it loads them."""
        d, v = self.d_model, self.P("transformer.wte.weight").shape[0]
        gemm, wp = (ops.gemm_nt_packed_bf16, self._wp16) if self._bf16_step else (ops.gemm_nt_packed, self._wp)
        for i in range(self.n_layer):
            q = f"transformer.h.{i}."
            a = ops.layernorm_fwd_packed(h, self.P(q + "ln_1.weight"), self.P(q + "ln_1.bias"), 1e-5)
            qkv = gemm(a, wp(q + "attn.c_attn.weight"), rows, 3 * d, d, b=self.P(q + "attn.c_attn.bias"))
            o = ops.attn_decode(qkv, state.k[i][:rows], state.v[i][:rows], key_mask, t, ancestry=state.anc,
                                out_packed=True)
            h = gemm(o, wp(q + "attn.c_proj.weight"), rows, d, d, b=self.P(q + "attn.c_proj.bias"), res=h)
            m = ops.layernorm_fwd_packed(h, self.P(q + "ln_2.weight"), self.P(q + "ln_2.bias"), 1e-5)
            f = gemm(m, wp(q + "mlp.c_fc.weight"), rows, 4 * d, d, b=self.P(q + "mlp.c_fc.bias"),
                     act=ops.ACT_GELU_NEW, y_packed=True)
            h = gemm(f, wp(q + "mlp.c_proj.weight"), rows, d, 4 * d, b=self.P(q + "mlp.c_proj.bias"), res=h)
        state.len = t + 1
        hf = ops.layernorm_fwd_packed(h, self.P("transformer.ln_f.weight"), self.P("transformer.ln_f.bias"), 1e-5)
        return gemm(hf, wp("transformer.wte.weight", transposed=False), rows, v, d)

    @torch.no_grad()
    def generate_greedy(self, input_ids, max_length, pad_token_id, eos_token_id, sync_every=8):
        """huggingface `generate(num_beams=1, do_sample=False, use_cache=True)` as `Simple_GPT2.forward_gen`
        calls it (mdl_sf_base.py:494-503, 577-585): argmax of the newest position on the cached decode
        step, rows that have emitted eos receive pad from then on, and the result ends at the step where
        the last row finished (or at max_length).  The all-finished test reads the device only every
        `sync_every` steps; columns generated past the stopping step are cut off afterwards, so the result
        is the one of a loop testing after every token.  -> i64 [rows, <= max_length]"""
        rows, plen = input_ids.shape
        if not input_ids.is_cuda:
            raise ops._lib.VsError("GPT-2 runs on the HIP kernels only (GPU tensor required)")
        if not 1 <= plen <= max_length <= self.n_positions:
            raise ops._lib.VsError(f"prompt {plen} / max_length {max_length} / n_positions {self.n_positions}")
        state = KVCacheState()
        out = torch.full((rows, max_length), pad_token_id, dtype=torch.int64, device=input_ids.device)
        out[:, :plen] = input_ids
        unfinished = torch.ones(rows, dtype=torch.bool, device=input_ids.device)
        alive = torch.ones(max_length, dtype=torch.bool, device=input_ids.device)  # any row unfinished after col t
        logits = None
        for t in range(plen):  # the prompt, one cached position at a time (prompts here are one token)
            logits = self.forward_step(input_ids[:, t].contiguous(), state, max_len=max_length)
        end = max_length
        for t in range(plen, max_length):
            _, nxt = ops.softmax_topk(logits, 1)
            add = torch.where(unfinished, nxt[:, 0], torch.full_like(nxt[:, 0], pad_token_id))
            out[:, t] = add
            unfinished = unfinished & add.ne(eos_token_id)
            alive[t] = unfinished.any()
            if (t - plen) % sync_every == sync_every - 1 or t == max_length - 1:
                dead = (~alive[plen:t + 1]).nonzero()
                if dead.numel():
                    end = plen + int(dead[0]) + 1
                    break
            if t + 1 < max_length:
                logits = self.forward_step(add, state, max_len=max_length)
        return out[:, :end].contiguous()

    # ---- training (teacher-forced pass with saved activations + manual backward) ------------
    def forward_train(self, tokens, attention_mask=None):
        """Like forward_logits, keeping what the backward needs (fp32, no recompute except the
        attention probabilities)."""
        r, l = tokens.shape
        km = None if attention_mask is None else attention_mask.to(torch.uint8).contiguous()
        # the step's [seed, step] snapshot: every mask of this forward and of its backward is a function of it
        snap = ops.dropout_tick(self._drop_state_on(tokens.device)) if self._dropout_on() else None
        h = ops.gpt2_embed(tokens, self.P("transformer.wte.weight"), self.P("transformer.wpe.weight"),
                           drop=self._site(snap, 0, self._drop_embd))
        layers = []
        for i in range(self.n_layer):
            q = f"transformer.h.{i}."
            a, mean1, rstd1 = ops.add_layernorm_fwd(h, None, self.P(q + "ln_1.weight"),
                                                    self.P(q + "ln_1.bias"), 1e-5)
            qkv = ops.gemm_nt(a, self._w(q + "attn.c_attn.weight"), self.P(q + "attn.c_attn.bias"), bf16=self._bf16)
            o = ops.attn_causal(qkv, km, r, l, self.n_head, drop=self._site(snap, 1 + 3 * i, self._drop_attn))
            h_mid = self._proj_res(q + "attn.c_proj", o, h, self._site(snap, 2 + 3 * i, self._drop_resid))
            m, mean2, rstd2 = ops.add_layernorm_fwd(h_mid, None, self.P(q + "ln_2.weight"),
                                                    self.P(q + "ln_2.bias"), 1e-5)
            f_pre = ops.gemm_nt(m, self._w(q + "mlp.c_fc.weight"), self.P(q + "mlp.c_fc.bias"), bf16=self._bf16)
            f = ops.gelu_new_fwd(f_pre)
            h_out = self._proj_res(q + "mlp.c_proj", f, h_mid, self._site(snap, 3 + 3 * i, self._drop_resid))
            layers.append((h, a, mean1, rstd1, qkv, o, h_mid, m, mean2, rstd2, f_pre, f))
            h = h_out
        hf, meanf, rstdf = ops.add_layernorm_fwd(h, None, self.P("transformer.ln_f.weight"),
                                                 self.P("transformer.ln_f.bias"), 1e-5)
        logits = ops.gemm_nt(hf, self.P("transformer.wte.weight"), bf16=self._bf16)
        self._saved = (tokens, km, r, l, layers, h, hf, meanf, rstdf, snap)
        return logits.view(r, l, -1)

    def _proj_res(self, name, x, res, drop):
        """res + dropout(x W + b): at a dropout site the GEMM runs without the residual and the mask kernel adds it
        (the GEMM epilogues and the split-K reduce stay as they are)."""
        if drop is None:
            return ops.gemm_nt(x, self._w(name + ".weight"), self.P(name + ".bias"), res=res, bf16=self._bf16)
        return ops.dropout_add(ops.gemm_nt(x, self._w(name + ".weight"), self.P(name + ".bias"), bf16=self._bf16),
                               res, drop)

    @torch.no_grad()
    def backward(self, dlogits):
        """dlogits [R*L, V] -> .grad of every parameter (overwrite semantics, like the trunk)."""
        tokens, km, r, l, layers, h_last, hf, meanf, rstdf, snap = self._saved
        self._saved = None
        wte = self.P("transformer.wte.weight")
        dlogits = dlogits.reshape(r * l, -1)
        # tied lm_head: logits = hf @ wte^T
        dwte = self._grad("transformer.wte.weight")
        ops.gemm_nt(ops.transpose_f32(dlogits), ops.transpose_f32(hf), out=dwte, bf16=self._bf16)
        dhf = ops.gemm_nt(dlogits, ops.transpose_f32(wte), bf16=self._bf16)
        dh, _, _, _ = ops.add_layernorm_bwd(dhf, h_last, None, self.P("transformer.ln_f.weight"), meanf,
                                            rstdf, dg_out=self._grad("transformer.ln_f.weight"),
                                            db_out=self._grad("transformer.ln_f.bias"))
        for i in reversed(range(self.n_layer)):
            q = f"transformer.h.{i}."
            h_in, a, mean1, rstd1, qkv, o, h_mid, m, mean2, rstd2, f_pre, f = layers[i]
            s_attn, s_proj, s_mlp = (self._site(snap, k + 3 * i, p) for k, p in
                                     ((1, self._drop_attn), (2, self._drop_resid), (3, self._drop_resid)))
            df = self._linear_bwd(q + "mlp.c_proj", f, dh if s_mlp is None else ops.dropout_add(dh, None, s_mlp),
                                  conv1d=True, bf16=self._bf16)
            df_pre = ops.gelu_new_bwd(df, f_pre)
            dm = self._linear_bwd(q + "mlp.c_fc", m, df_pre, conv1d=True, bf16=self._bf16)
            dmid_ln, _, _, _ = ops.add_layernorm_bwd(dm, h_mid, None, self.P(q + "ln_2.weight"), mean2, rstd2,
                                                     dg_out=self._grad(q + "ln_2.weight"),
                                                     db_out=self._grad(q + "ln_2.bias"))
            d_mid = ops.add_f32(dh, dmid_ln)
            do = self._linear_bwd(q + "attn.c_proj", o,
                                  d_mid if s_proj is None else ops.dropout_add(d_mid, None, s_proj), conv1d=True,
                                  bf16=self._bf16)
            dqkv = ops.attn_causal_bwd(qkv, km, do, r, l, self.n_head, drop=s_attn)
            da = self._linear_bwd(q + "attn.c_attn", a, dqkv, conv1d=True, bf16=self._bf16)
            din_ln, _, _, _ = ops.add_layernorm_bwd(da, h_in, None, self.P(q + "ln_1.weight"), mean1, rstd1,
                                                    dg_out=self._grad(q + "ln_1.weight"),
                                                    db_out=self._grad(q + "ln_1.bias"))
            dh = ops.add_f32(d_mid, din_ln)
            layers[i] = None
        dwpe = self._grad("transformer.wpe.weight")
        dwpe.zero_()
        s_embd = self._site(snap, 0, self._drop_embd)
        if s_embd is not None:
            dh = ops.dropout_add(dh, None, s_embd)
        ops.gpt2_embed_bwd(tokens, dh, dwte, dwpe)  # adds the embedding rows onto the lm_head gradient
        self._drop_copies()  # the optimizer is about to change the parameters

    def reorder_state(self, state: KVCacheState, new_order):
        """fairseq reorder_incremental_state: row r of the cache becomes old row new_order[r]."""
        state.reorder(new_order, self.n_layer)


_GPT2TrainFn = FlatTrainFn  # the name tests/test_gpu_gpt2.py imports


class _XentIgnoreFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits2d, labels, ignore_index):
        loss, pair = ops.xent_ignore(logits2d, labels, ignore_index)
        ctx.save_for_backward(logits2d, labels, pair)
        ctx.ignore_index = ignore_index
        return loss.clone()

    @staticmethod
    def backward(ctx, go):
        logits2d, labels, pair = ctx.saved_tensors
        return ops.xent_ignore_grad(logits2d, labels, pair, ctx.ignore_index, go), None, None  # go stays on the device


class HuggingFaceGPT2Decoder(nn.Module):
    """hf_gpt2_fseq.py:124-215.  `args` is the full config (`args.mdl.gpt2_mdl_name`), `dictionary`
    the tokenizer object (`pad()`, `eos()`, `__len__`)."""

    # `forward` never reads encoder_out (hf_gpt2_fseq.py:165-203 does not either): decode steps may be
    # captured in hipGraphs without pinning the encoder output's address
    uses_encoder_out = False

    def __init__(self, args, dictionary, state_dict=None):
        super().__init__()
        self.dictionary = dictionary
        dims = GPT2_DIMS[args.mdl.gpt2_mdl_name]
        # one number for the three probabilities, as hf_gpt2_fseq.py:144-146 intended; absent in the reference's
        # own config file, hence the default
        pdrop = float(args.mdl.get("gpt2_dropout", 0.0))
        # "fp32" | "bf16": operand precision of the whole-sequence GEMMs (this project's own switch)
        self.model = GPT2LMHeadModelHip(*dims, embd_pdrop=pdrop, attn_pdrop=pdrop, resid_pdrop=pdrop,
                                        matmul=str(args.mdl.get("gpt2_matmul", "fp32")),
                                        decode_matmul=str(args.mdl.get("gpt2_decode_matmul", "fp32")))
        if state_dict is not None:
            self.model.load_state_dict(state_dict)
        self.voc_size = len(dictionary)
        self.model.resize_token_embeddings(self.voc_size)
        self.pad_idx = dictionary.pad()

    def forward(self, prev_output_tokens, src_lengths=None, incremental_state=None, encoder_out=None):
        if incremental_state:  # cached single-position step (see module docstring)
            if incremental_state.len != prev_output_tokens.size(1) - 1:
                raise ops._lib.VsError("incremental state out of step with prev_output_tokens")
            logits = self.model.forward_step(prev_output_tokens[:, -1].contiguous(), incremental_state,
                                             max_len=getattr(incremental_state, "max_len", None))
            return (logits.unsqueeze(1),)
        features_mask = prev_output_tokens.ne(self.pad_idx)  # don't attend to padding symbols (:185)
        if self.training and torch.is_grad_enabled():
            tick = torch.zeros(1, device=prev_output_tokens.device, requires_grad=True)
            return (FlatTrainFn.apply(self.model, prev_output_tokens, features_mask, tick),)
        return (self.model.forward_logits(prev_output_tokens, features_mask),)

    def reorder_incremental_state(self, incremental_state, new_order):
        if incremental_state:
            self.model.reorder_state(incremental_state, new_order)

    def max_positions(self):
        return self.model.config.n_positions - 1

    def max_decoder_positions(self):
        return self.model.config.n_positions - 1


def lm_loss(logits, tokens, pad_index):
    """`Simple_TxDec.forward` (`mdl_sf_base.py:653-667`): CE(logits[:, :-1], tokens[:, 1:]),
    ignore_index = pad, mean over the counted tokens."""
    r, l, v = logits.shape
    labels = torch.full((r, l), pad_index, dtype=torch.int64, device=tokens.device)
    labels[:, :-1] = tokens[:, 1:]
    if logits.requires_grad:
        return _XentIgnoreFn.apply(logits.reshape(r * l, v), labels.reshape(-1), pad_index)
    loss, _ = ops.xent_ignore(logits.reshape(r * l, v), labels.reshape(-1), pad_index)
    return loss
