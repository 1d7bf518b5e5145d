"""Plain torch restatement of the RoBERTa encoder with bf16-operand dense layers (`matmul="bf16"`), in any dtype:
`roberta_ref.encoder` built from the same functions (embed, layer_norm, attention, gelu), where each dense layer of the
encoder stack -- query, key, value, attention.output.dense, intermediate.dense, output.dense -- is ONE autograd function
that rounds both operands of each of its three products to bf16: x and W in the forward, dy and W for dx, dy and x for
dW.  Sums, biases, the bias gradient and everything between the dense layers stay in the working dtype; the pooler and
the classification head are `roberta_ref`'s (they stay fp32 in the model).  `rnd=False` switches the rounding off: the
function is then a plain dense layer and `encoder` equals `roberta_ref.encoder`.

`round_bf16` is tests/gpt2_bf16_ref.py's: nearest, ties to even, by integer arithmetic on the fp32 bit pattern."""
import torch

import roberta_ref as ref
from gpt2_bf16_ref import round_bf16


class DenseBf16(torch.autograd.Function):
    """y = r(x) r(W)^T + b for x [..., in], W [out, in]; dx = r(dy) r(W), dW = r(dy)^T r(x), db = sum dy."""

    @staticmethod
    def forward(ctx, x, w, b, rnd):
        r = round_bf16 if rnd else (lambda v: v)
        ctx.save_for_backward(x, w)
        ctx.r = r
        return r(x) @ r(w).t() + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        r = ctx.r
        x2, dy2 = x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])
        dx = (r(dy2) @ r(w)).view(x.shape)
        dw = r(dy2).t() @ r(x2)
        return dx, dw, dy2.sum(0), None


def encoder(w, tokens, mask, dims, prefix="", rnd=True):
    """-> last hidden state [R, L, D]."""
    eps, nh = dims["layer_norm_eps"], dims["n_head"]

    def lin(x, name):
        return DenseBf16.apply(x, w[prefix + name + ".weight"], w[prefix + name + ".bias"], rnd)

    def ln(x, name):
        return ref.layer_norm(x, w[prefix + name + ".weight"], w[prefix + name + ".bias"], eps)

    e, _ = ref.embed(w, tokens, dims, prefix)
    h = ln(e, "embeddings.LayerNorm")
    for i in range(dims["n_layer"]):
        q = f"encoder.layer.{i}."
        qkv = torch.cat([lin(h, q + "attention.self." + s) for s in ("query", "key", "value")], dim=-1)
        ctx = ref.attention(qkv, mask, nh)
        h = ln(lin(ctx, q + "attention.output.dense") + h, q + "attention.output.LayerNorm")
        f = ref.gelu(lin(h, q + "intermediate.dense"))
        h = ln(lin(f, q + "output.dense") + h, q + "output.LayerNorm")
    return h
