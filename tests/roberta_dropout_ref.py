"""Plain-torch restatement of the RoBERTa encoder, its pooler and the classification head in train mode: dropout
enters as mask operands (tensors of 0 or 1 / (1 - p), any dtype), so fp64 is the yardstick and fp32 the restatement's
own noise floor, exactly as tests/roberta_ref.py is for the model without dropout.  Built on roberta_ref (the
architecture) and dropout_ref (the generator contract); with every mask None each function here is roberta_ref's.

Dropout sites of the pinned transformers release (3.3.1, modeling_roberta / modeling_bert), n layers:

  site 0          the embeddings after their LayerNorm                       hidden probability   [R*L, D] flat
  site 1 + 3i     layer i: the attention probabilities                       attention probability
                  element ((r*H + h)*L + q)*Lp4 + k, Lp4 = (L + 3) & ~3      (dropout_ref.keep_attn)
  site 2 + 3i     layer i: attention.output.dense before its LayerNorm       hidden probability   [R*L, D] flat
  site 3 + 3i     layer i: output.dense before its LayerNorm                 hidden probability   [R*L, D] flat
  site 1 + 3n     head: h[:, 0] before classifier.dense                      hidden probability   [R, D] flat
  site 2 + 3n     head: after the tanh, before classifier.out_proj           hidden probability   [R, D] flat

The pooler has no dropout.
"""
import math

import torch

import dropout_ref
import roberta_ref as ref


def site_list(n_layer, head=False):
    """[(site number, "hidden" | "attention", where)] in the order the forward meets them."""
    sites = [(0, "hidden", "embeddings")]
    for i in range(n_layer):
        sites += [(1 + 3 * i, "attention", f"layer {i} attention probabilities"),
                  (2 + 3 * i, "hidden", f"layer {i} attention.output.dense"),
                  (3 + 3 * i, "hidden", f"layer {i} output.dense")]
    if head:
        sites += [(1 + 3 * n_layer, "hidden", "classifier.dense input"),
                  (2 + 3 * n_layer, "hidden", "classifier.out_proj input")]
    return sites


def masks(seed, step, dims, r, l, p_hidden, p_attention, head=False):
    """{site: fp64 multiplier tensor | None (probability 0)} for one step; shapes [R, L, D], [R, H, L, L], [R, D]."""
    d, nh = dims["d_model"], dims["n_head"]
    out = {}
    for site, kind, where in site_list(dims["n_layer"], head):
        p = p_hidden if kind == "hidden" else p_attention
        if p == 0.0:
            out[site] = None
            continue
        thr, scale = dropout_ref.threshold(p)
        if kind == "attention":
            keep = dropout_ref.keep_attn(seed, step, site, r, nh, l, thr)
        elif where.startswith("classifier"):
            keep = dropout_ref.keep_flat(seed, step, site, r * d, thr).reshape(r, d)
        else:
            keep = dropout_ref.keep_flat(seed, step, site, r * l * d, thr).reshape(r, l, d)
        out[site] = torch.from_numpy(keep).double() * scale
    return out


def _drop(x, m):
    return x if m is None else x * m.to(x.dtype)


def attention(qkv, mask, n_head, keep=None):
    """roberta_ref.attention with the probabilities multiplied by `keep` [R, H, L, L] after the softmax."""
    r, l, d3 = qkv.shape
    d = d3 // 3
    dh = d // n_head
    q, k, v = (t.reshape(r, l, n_head, dh).transpose(1, 2) for t in qkv.split(d, dim=-1))
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    if mask is not None:
        s = s + (1.0 - mask.to(qkv.dtype))[:, None, None, :] * -1e4
    p = _drop(torch.softmax(s, dim=-1), keep)
    return (p @ v).transpose(1, 2).reshape(r, l, d)


def add_layernorm(b, res, g, beta, eps, m=None):
    """LayerNorm(res + m * b) -> (y, mean, rstd), the residual site on its own."""
    s = _drop(b, m) + res
    mu = s.mean(-1, keepdim=True)
    var = ((s - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (s - mu) * rstd * g + beta, mu.squeeze(-1), rstd.squeeze(-1)


def encoder(w, tokens, mask, dims, drops, prefix=""):
    """-> last hidden state [R, L, D]; drops: what `masks` returns ({} = no dropout)."""
    eps, nh = dims["layer_norm_eps"], dims["n_head"]

    def lin(x, name):
        return x @ w[prefix + name + ".weight"].t() + w[prefix + name + ".bias"]

    def ln(x, name):
        return ref.layer_norm(x, w[prefix + name + ".weight"], w[prefix + name + ".bias"], eps)

    e, _ = ref.embed(w, tokens, dims, prefix)
    h = _drop(ln(e, "embeddings.LayerNorm"), drops.get(0))
    for i in range(dims["n_layer"]):
        q = f"encoder.layer.{i}."
        qkv = torch.cat([lin(h, q + "attention.self." + s) for s in ("query", "key", "value")], dim=-1)
        ctx = attention(qkv, mask, nh, drops.get(1 + 3 * i))
        h = ln(_drop(lin(ctx, q + "attention.output.dense"), drops.get(2 + 3 * i)) + h, q + "attention.output.LayerNorm")
        f = ref.gelu(lin(h, q + "intermediate.dense"))
        h = ln(_drop(lin(f, q + "output.dense"), drops.get(3 + 3 * i)) + h, q + "output.LayerNorm")
    return h


pooler = ref.pooler  # no dropout


def classifier(w, h, drops, n_layer):
    x = _drop(h[:, 0], drops.get(1 + 3 * n_layer))
    c = torch.tanh(x @ w["classifier.dense.weight"].t() + w["classifier.dense.bias"])
    c = _drop(c, drops.get(2 + 3 * n_layer))
    return c @ w["classifier.out_proj.weight"].t() + w["classifier.out_proj.bias"]
