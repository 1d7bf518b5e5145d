"""RoBERTa encoder of the event-relation models (`vidsitu_code/mdl_evrel.py:21,62`) on the HIP kernels of
csrc/roberta_ops.hip and the fp32 GEMM / LayerNorm kernels the GPT-2 path already uses.

The reference builds `RobertaForSequenceClassification.from_pretrained(cfg.mdl.rob_mdl_name, num_labels=5)` and
`RobertaModel.from_pretrained(..., add_pooling_layer=True)` (huggingface transformers==3.3.1); there is no network here,
so `RobertaModelHip` / `RobertaForSequenceClassificationHip` are built from the architecture's dimensions with random
weights and load a huggingface state dict when one is given (same keys and shapes; the `embeddings.position_ids` buffer
that checkpoints of the pinned release carry is ignored).

Semantics kept from the pinned release: additive key mask `(1 - attention_mask) * -1e4`, position ids from the token
ids (`create_position_ids_from_input_ids`: padding tokens sit at `padding_idx`, the others count from `padding_idx + 1`),
the single token-type row, post-LN residual blocks, erf GELU, LayerNorm eps 1e-5 (the checkpoints' value), pooler
`tanh(dense(h[:, 0]))`, classification head `out_proj(tanh(dense(h[:, 0])))`.

Dropout: `from_pretrained` gives the reference huggingface's defaults (`hidden_dropout_prob =
attention_probs_dropout_prob = 0.1`); here both are constructor arguments, 0 by default (`mdl.rob_dropout` sets them).
Above 0 the train-mode pass applies the masks of the pinned release's dropout sites from the counter generator of
csrc/dropout_rng.h inside the kernels; nothing is stored, the backward regenerates them from the step's `[seed, step]`
snapshot, which travels with the saved activations.  Site numbers (n layers): 0 the embeddings after their LayerNorm;
layer i: 1 + 3i the attention probabilities, 2 + 3i `attention.output.dense` before its LayerNorm, 3 + 3i
`output.dense` before its LayerNorm; classification head: 1 + 3n on `h[:, 0]` before `classifier.dense`, 2 + 3n after
the tanh before `out_proj`; the pooler has none.  `forward()` and `roberta_apply` outside training never apply dropout
and never advance the state; at every probability 0 the model issues the launches it issued without the arguments.

Training: `forward_train` keeps the activations, `backward` is a manual HIP backward behind ONE autograd node
(`roberta_apply` -> `flat_module.FlatTrainFn`); parameter gradients are written with overwrite semantics.  Flat
registration, the state-dict rules, the fused q/k/v cache's life and the dense-layer backward are `FlatParamModule`'s.

`matmul="bf16"` (`mdl.rob_matmul`): the encoder's dense layers -- the fused q/k/v projection, `attention.output.dense`,
`intermediate.dense`, `output.dense` -- take bf16 operands with fp32 accumulation, in training and in the plain forward
alike.  Activations and weights stay fp32 in memory and are rounded inside the GEMM's loader.  The backward's products
go through `ops.gemm_bf16`, whose K-strided operand forms read dy, x and W where they lie: no transposed copy of any
of them exists in that mode, and the cached transposed q/k/v weight is not built.  Parameters, Adam, the embeddings,
LayerNorm, attention, GELU, dropout, bias gradients, the pooler and the classification head (a handful of rows) stay
fp32.  The default "fp32" issues the launches it issued before the argument existed.
"""
import torch
from torch import nn

from . import ops
from .flat_module import FlatParamModule, FlatTrainFn

ROBERTA_DIMS = {
    # name: dict(n_layer, d_model, n_head, n_positions, vocab, d_ffn, pad, eps)
    "roberta-base": dict(n_layer=12, d_model=768, n_head=12, n_positions=514, vocab_size=50265, d_ffn=3072,
                         pad_token_id=1, layer_norm_eps=1e-5),
    "roberta-synth-tiny": dict(n_layer=2, d_model=64, n_head=2, n_positions=130, vocab_size=101, d_ffn=128,
                               pad_token_id=1, layer_norm_eps=1e-5),  # tests / main_dist on synthetic data
}


class _RobertaHip(FlatParamModule):
    """Parameters under huggingface's names, the encoder's forward / backward."""

    PREFIX = ""
    # layer -> ([3D][D] weight, [3D] bias, [D][3D] transposed weight | None in bf16 mode): one GEMM for q, k and v
    _CACHES = ("_qkv",)
    _CAPTURE_MSG = "RoBERTa's fused q/k/v weights must exist before a graph capture (run one eager step first)"
    _DROP_CAPTURE_MSG = "the RoBERTa dropout state must exist before a graph capture (run one eager step first)"

    def __init__(self, n_layer, d_model, n_head, n_positions, vocab_size, d_ffn, pad_token_id=1, layer_norm_eps=1e-5,
                 add_pooling_layer=True, num_labels=0, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                 matmul="fp32"):
        super().__init__()
        if matmul not in ("fp32", "bf16"):
            raise ValueError(f"matmul must be 'fp32' or 'bf16', got {matmul!r}")
        self.matmul = matmul
        self._bf16 = matmul == "bf16"  # the encoder's dense layers only
        if d_model % n_head:
            raise ValueError("d_model must be a multiple of n_head")
        self.hidden_dropout_prob = float(hidden_dropout_prob)
        self.attention_probs_dropout_prob = float(attention_probs_dropout_prob)
        # (thr, scale) per probability, None at p = 0 (that site then runs today's launches); refuses p outside [0, 1)
        self._drop_hid, self._drop_att = (ops.dropout_params(p) if p != 0.0 else None
                                          for p in (hidden_dropout_prob, attention_probs_dropout_prob))
        self.n_layer, self.d_model, self.n_head, self.n_positions = n_layer, d_model, n_head, n_positions
        self.d_ffn, self.pad, self.eps = d_ffn, pad_token_id, layer_norm_eps
        self.has_pooler, self.num_labels = bool(add_pooling_layer), int(num_labels)
        self.config = type("Cfg", (), dict(num_hidden_layers=n_layer, hidden_size=d_model, num_attention_heads=n_head,
                                           max_position_embeddings=n_positions, vocab_size=vocab_size,
                                           intermediate_size=d_ffn, pad_token_id=pad_token_id,
                                           layer_norm_eps=layer_norm_eps, type_vocab_size=1, num_labels=num_labels))()
        p = {}
        pre = self.PREFIX

        def add(name, *shape, std=0.02, ones=False):
            t = torch.ones(*shape) if ones else (torch.randn(*shape) * std if std else torch.zeros(*shape))
            p[pre + name] = nn.Parameter(t)

        def dense(name, n_out, n_in):
            add(name + ".weight", n_out, n_in)
            add(name + ".bias", n_out, std=0)

        def lnorm(name):
            add(name + ".weight", d_model, ones=True)
            add(name + ".bias", d_model, std=0)

        add("embeddings.word_embeddings.weight", vocab_size, d_model)
        add("embeddings.position_embeddings.weight", n_positions, d_model)
        add("embeddings.token_type_embeddings.weight", 1, d_model)
        with torch.no_grad():  # nn.Embedding(padding_idx): the row starts at zero (and never receives a gradient)
            p[pre + "embeddings.word_embeddings.weight"][pad_token_id].zero_()
            p[pre + "embeddings.position_embeddings.weight"][pad_token_id].zero_()
        lnorm("embeddings.LayerNorm")
        for i in range(n_layer):
            q = f"encoder.layer.{i}."
            for s in ("query", "key", "value"):
                dense(q + "attention.self." + s, d_model, d_model)
            dense(q + "attention.output.dense", d_model, d_model)
            lnorm(q + "attention.output.LayerNorm")
            dense(q + "intermediate.dense", d_ffn, d_model)
            dense(q + "output.dense", d_model, d_ffn)
            lnorm(q + "output.LayerNorm")
        if self.has_pooler:
            dense("pooler.dense", d_model, d_model)
        if self.num_labels:  # RobertaClassificationHead lives beside the encoder, not under its prefix
            for name, (n_out, n_in) in (("classifier.dense", (d_model, d_model)),
                                        ("classifier.out_proj", (self.num_labels, d_model))):
                p[name + ".weight"] = nn.Parameter(torch.randn(n_out, n_in) * 0.02)
                p[name + ".bias"] = nn.Parameter(torch.zeros(n_out))
        self._register_flat(p)

    # ---- huggingface-compatible state dict -------------------------------------------------
    def E(self, name):
        """A parameter of the encoder (under the model's prefix)."""
        return self.P(self.PREFIX + name)

    def _tolerated_on_load(self, key):
        # checkpoints of the pinned release carry the position-id buffer; newer releases dropped it
        return key.endswith("embeddings.position_ids")

    def _fused_qkv(self, i):
        q = f"encoder.layer.{i}.attention.self."

        def make():
            w = torch.cat([self.E(q + s + ".weight").detach() for s in ("query", "key", "value")], 0).contiguous()
            b = torch.cat([self.E(q + s + ".bias").detach() for s in ("query", "key", "value")], 0).contiguous()
            return w, b, None if self._bf16 else ops.transpose_f32(w)  # bf16: dx reads w itself (K-strided)

        return self._copy(self._qkv, i, self.E(q + "query.weight"), make)

    # ---- compute ---------------------------------------------------------------------------
    def _check(self, tokens, attention_mask):
        if not tokens.is_cuda:
            raise ops._lib.VsError("RoBERTa runs on the HIP kernels only (GPU tensor required)")
        if tokens.dim() != 2:
            raise ops._lib.VsError("input_ids must be [R, L]")
        if attention_mask is None:
            return None
        if attention_mask.shape != tokens.shape:
            raise ops._lib.VsError("attention_mask must have the shape of input_ids")
        return attention_mask.ne(0).to(torch.uint8).contiguous()

    def _dense(self, name, x):
        return ops.gemm_nt(x, self.E(name + ".weight"), self.E(name + ".bias"))

    def _enc_dense(self, name, x):
        """A dense layer of the encoder stack: the one place `matmul` acts in the forward (beside the fused q/k/v)."""
        return ops.gemm_nt(x, self.E(name + ".weight"), self.E(name + ".bias"), bf16=self._bf16)

    def _enc_linear_bwd(self, name, x, dy):
        return self._linear_bwd(name, x, dy, direct=self._bf16)

    def _tick(self, tokens, keep):
        """The [seed, step] snapshot of a train-mode pass with dropout (one tick); None otherwise."""
        if not keep or (self._drop_hid is None and self._drop_att is None):
            return None
        return ops.dropout_tick(self._drop_state_on(tokens.device))

    def _ln_site(self, b, res, name, drop):
        """LayerNorm(res + dropout(b)) -> (b | the sum, y, mean, rstd).  At a dropout site the mask kernel forms
        s = res + m o b and the LayerNorm runs on s alone; s is what the backward keeps in b's place (a kernel pair that
        draws the mask inside the LayerNorm passes was built and measured slower: DESIGN.md, "RoBERTa dropout")."""
        g, bt = self.E(name + ".weight"), self.E(name + ".bias")
        if drop is None:
            return (b,) + ops.add_layernorm_fwd(b, res, g, bt, self.eps)
        s = ops.dropout_add(b, res, drop)
        return (s,) + ops.add_layernorm_fwd(s, None, g, bt, self.eps)

    def _ln_site_bwd(self, dy, b, res, name, mean, rstd, drop):
        """-> (d_res, d_b) of `_ln_site` (b: what it returned first); the LayerNorm's parameter gradients are written."""
        dg, db = self._grad(name + ".weight"), self._grad(name + ".bias")
        if drop is None:
            ds = ops.add_layernorm_bwd(dy, b, res, self.P(name + ".weight"), mean, rstd, dg_out=dg, db_out=db)[0]
            return ds, ds
        ds = ops.add_layernorm_bwd(dy, b, None, self.P(name + ".weight"), mean, rstd, dg_out=dg, db_out=db)[0]
        return ds, ops.dropout_add(ds, None, drop)

    def _encode(self, tokens, attention_mask, keep, snap=None):
        """-> (last hidden state [R*L, D], saved activations | None).  snap: the step's dropout snapshot or None."""
        km = self._check(tokens, attention_mask)
        hid = None if snap is None else self._drop_hid
        att = None if snap is None else self._drop_att
        r, l = tokens.shape
        e, pos_ids = ops.roberta_embed(tokens, self.E("embeddings.word_embeddings.weight"),
                                       self.E("embeddings.position_embeddings.weight"),
                                       self.E("embeddings.token_type_embeddings.weight"), self.pad)
        h, mean0, rstd0 = ops.add_layernorm_fwd(e, None, self.E("embeddings.LayerNorm.weight"),
                                                self.E("embeddings.LayerNorm.bias"), self.eps)
        if hid is not None:
            h = ops.dropout_add(h, None, self._site(snap, 0, hid))
        layers = []
        for i in range(self.n_layer):
            q = f"encoder.layer.{i}."
            w, b, _ = self._fused_qkv(i)
            qkv = ops.gemm_nt(h, w, b, bf16=self._bf16)
            ctx = ops.attn_pad(qkv, km, r, l, self.n_head, drop=self._site(snap, 1 + 3 * i, att))
            ao = self._enc_dense(q + "attention.output.dense", ctx)
            ao, h1, mean1, rstd1 = self._ln_site(ao, h, q + "attention.output.LayerNorm",
                                                 self._site(snap, 2 + 3 * i, hid))
            f_pre = self._enc_dense(q + "intermediate.dense", h1)
            f = ops.gelu_erf_fwd(f_pre)
            fo = self._enc_dense(q + "output.dense", f)
            fo, h2, mean2, rstd2 = self._ln_site(fo, h1, q + "output.LayerNorm", self._site(snap, 3 + 3 * i, hid))
            if keep:
                layers.append((h, qkv, ctx, ao, mean1, rstd1, h1, f_pre, f, fo, mean2, rstd2))
            h = h2
        saved = (tokens, pos_ids, km, r, l, e, mean0, rstd0, layers, snap) if keep else None
        return h, saved

    def _first_token(self, h, r, l):
        return h.view(r, l, self.d_model)[:, 0].contiguous()

    def _encode_bwd(self, saved, dh):
        """dh [R*L, D]: gradient of the last hidden state -> every encoder / embedding parameter's .grad."""
        tokens, pos_ids, km, r, l, e, mean0, rstd0, layers, snap = saved
        d, pre = self.d_model, self.PREFIX  # parameters by their full names from here on
        hid = None if snap is None else self._drop_hid
        att = None if snap is None else self._drop_att
        for i in reversed(range(self.n_layer)):
            q = f"{pre}encoder.layer.{i}."
            h_in, qkv, ctx, ao, mean1, rstd1, h1, f_pre, f, fo, mean2, rstd2 = layers[i]
            ds2, dfo = self._ln_site_bwd(dh, fo, h1, q + "output.LayerNorm", mean2, rstd2,
                                         self._site(snap, 3 + 3 * i, hid))
            df = self._enc_linear_bwd(q + "output.dense", f, dfo)
            df_pre = ops.gelu_erf_bwd(df, f_pre)
            dh1 = ops.add_f32(self._enc_linear_bwd(q + "intermediate.dense", h1, df_pre), ds2)
            ds1, dao = self._ln_site_bwd(dh1, ao, h_in, q + "attention.output.LayerNorm", mean1, rstd1,
                                         self._site(snap, 2 + 3 * i, hid))
            dctx = self._enc_linear_bwd(q + "attention.output.dense", ctx, dao)
            dqkv = ops.attn_pad_bwd(qkv, km, dctx, r, l, self.n_head, drop=self._site(snap, 1 + 3 * i, att))
            # the fused projection: weight gradients straight into the three separate parameters
            w, _, wt = self._fused_qkv(i)
            if not self._bf16:
                dqkv_t, h_t = ops.transpose_f32(dqkv), ops.transpose_f32(h_in)
            db = ops.colsum_f32(dqkv)
            for s, nm in enumerate(("query", "key", "value")):
                dw = self._grad(q + "attention.self." + nm + ".weight")
                if self._bf16:  # a row range of dqkv^T is a column range of dqkv: a K-strided operand where it lies
                    ops.gemm_bf16(dqkv[:, s * d:(s + 1) * d], h_in, out=dw, a_t=True, b_t=True)
                else:
                    ops.gemm_nt(dqkv_t[s * d:(s + 1) * d], h_t, out=dw)
                self._grad(q + "attention.self." + nm + ".bias").copy_(db[s * d:(s + 1) * d])
            dx = ops.gemm_bf16(dqkv, w, b_t=True) if self._bf16 else ops.gemm_nt(dqkv, wt)
            dh = ops.add_f32(dx, ds1)
            layers[i] = None
        if hid is not None:
            dh = ops.dropout_add(dh, None, self._site(snap, 0, hid))
        de = ops.add_layernorm_bwd(dh, e, None, self.P(pre + "embeddings.LayerNorm.weight"), mean0, rstd0,
                                   dg_out=self._grad(pre + "embeddings.LayerNorm.weight"),
                                   db_out=self._grad(pre + "embeddings.LayerNorm.bias"))[0]
        dword = self._grad(pre + "embeddings.word_embeddings.weight")
        dpos = self._grad(pre + "embeddings.position_embeddings.weight")
        dword.zero_()
        dpos.zero_()
        # both tables have padding_idx = pad: vs_embed_scatter_bwd skips those rows
        ops.embed_scatter_bwd(tokens, de, dword, 1.0, self.pad)
        ops.embed_scatter_bwd(pos_ids, de, dpos, 1.0, self.pad)
        ops.colsum_f32(de, out=self._grad(pre + "embeddings.token_type_embeddings.weight").view(-1))
        self._drop_copies()  # the optimizer is about to change the parameters


class RobertaModelHip(_RobertaHip):
    """`RobertaModel(add_pooling_layer=True)`: `forward(input_ids, attention_mask)` -> object with
    `last_hidden_state` [R, L, D] and `pooler_output` [R, D]."""

    def __init__(self, *args, add_pooling_layer=True, **kw):
        super().__init__(*args, add_pooling_layer=add_pooling_layer, num_labels=0, **kw)

    def _outputs(self, tokens, attention_mask, keep):
        r, l = tokens.shape
        h, saved = self._encode(tokens, attention_mask, keep, self._tick(tokens, keep))
        pooled = None
        x0 = None
        if self.has_pooler:
            x0 = self._first_token(h, r, l)
            pooled = ops.tanh_fwd(self._dense("pooler.dense", x0))
        if keep:
            self._saved = (saved, x0, pooled)
        return h.view(r, l, self.d_model), pooled

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None, return_dict=True):
        h, pooled = self._outputs(input_ids, attention_mask, keep=False)
        return _Out(last_hidden_state=h, pooler_output=pooled)

    @torch.no_grad()
    def forward_train(self, input_ids, attention_mask=None):
        """-> (last_hidden_state, pooler_output), keeping what `backward` needs."""
        return self._outputs(input_ids, attention_mask, keep=True)

    @torch.no_grad()
    def backward(self, dhidden, dpooled=None):
        """Gradients of the two outputs (either may be None) -> .grad of every parameter that took part."""
        saved, x0, pooled = self._saved
        self._saved = None
        r, l = saved[3], saved[4]
        if dhidden is not None:
            dh = dhidden.reshape(r * l, self.d_model).contiguous().clone()
        else:
            dh = torch.zeros((r * l, self.d_model), dtype=torch.float32, device=saved[0].device)
        if dpooled is not None and self.has_pooler:
            dpre = ops.tanh_bwd(dpooled.contiguous(), pooled)
            dx0 = self._linear_bwd(self.PREFIX + "pooler.dense", x0, dpre)
            dh.view(r, l, self.d_model)[:, 0] += dx0
        self._encode_bwd(saved, dh)


class RobertaForSequenceClassificationHip(_RobertaHip):
    """`RobertaForSequenceClassification(num_labels)`: encoder without pooler under `roberta.`, head
    `classifier.out_proj(tanh(classifier.dense(h[:, 0])))`; `forward` -> object with `logits` [R, num_labels]."""

    PREFIX = "roberta."

    def __init__(self, *args, num_labels=2, **kw):
        super().__init__(*args, add_pooling_layer=False, num_labels=num_labels, **kw)

    def _outputs(self, tokens, attention_mask, keep):
        r, l = tokens.shape
        snap = self._tick(tokens, keep)
        h, saved = self._encode(tokens, attention_mask, keep, snap)
        s_in, s_out = self._head_sites(snap)
        x0 = self._first_token(h, r, l)
        if s_in is not None:
            x0 = ops.dropout_add(x0, None, s_in)
        c1 = ops.tanh_fwd(ops.gemm_nt(x0, self.P("classifier.dense.weight"), self.P("classifier.dense.bias")))
        c1d = c1 if s_out is None else ops.dropout_add(c1, None, s_out)
        logits = ops.gemm_nt(c1d, self.P("classifier.out_proj.weight"), self.P("classifier.out_proj.bias"))
        if keep:
            self._saved = (saved, x0, c1)  # x0 after its dropout; the tanh's output before the second one
        return (logits,)

    def _head_sites(self, snap):
        """The head's two dropout sites (on h[:, 0], after the tanh); (None, None) without dropout."""
        hid = None if snap is None else self._drop_hid
        n = self.n_layer
        return self._site(snap, 1 + 3 * n, hid), self._site(snap, 2 + 3 * n, hid)

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None, return_dict=True):
        return _Out(logits=self._outputs(input_ids, attention_mask, keep=False)[0])

    @torch.no_grad()
    def forward_train(self, input_ids, attention_mask=None):
        return self._outputs(input_ids, attention_mask, keep=True)

    @torch.no_grad()
    def backward(self, dlogits):
        saved, x0, c1 = self._saved
        self._saved = None
        r, l = saved[3], saved[4]
        s_in, s_out = self._head_sites(saved[-1])
        c1d = c1 if s_out is None else ops.dropout_add(c1, None, s_out)  # out_proj's input, masked again
        dc1 = self._linear_bwd("classifier.out_proj", c1d, dlogits.contiguous())
        if s_out is not None:
            dc1 = ops.dropout_add(dc1, None, s_out)
        dx0 = self._linear_bwd("classifier.dense", x0, ops.tanh_bwd(dc1, c1))
        if s_in is not None:
            dx0 = ops.dropout_add(dx0, None, s_in)
        dh = torch.zeros((r * l, self.d_model), dtype=torch.float32, device=dx0.device)
        dh.view(r, l, self.d_model)[:, 0] = dx0
        self._encode_bwd(saved, dh)


class _Out(dict):
    """The `return_dict=True` output: keys are attributes too."""

    __getattr__ = dict.get


def roberta_apply(model, tokens, mask):
    """The model's outputs as tensors autograd can differentiate through (training), or the plain forward's."""
    if model.training and torch.is_grad_enabled():
        tick = torch.zeros(1, device=tokens.device, requires_grad=True)
        return FlatTrainFn.apply(model, tokens, mask, tick)
    with torch.no_grad():
        outs = model._outputs(tokens, mask, keep=False)
    return tuple(o for o in outs if o is not None)


def build(name, cls, state_dict=None, **kw):
    """`cls(**ROBERTA_DIMS[name])`, loading `state_dict` when one is given (the `from_pretrained` of this package)."""
    if name not in ROBERTA_DIMS:
        raise NotImplementedError(f"rob_mdl_name={name}: known dimensions are {sorted(ROBERTA_DIMS)}")
    m = cls(**ROBERTA_DIMS[name], **kw)
    if state_dict is not None:
        m.load_state_dict(state_dict)
    return m
