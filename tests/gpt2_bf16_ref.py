"""Plain torch restatement of the GPT-2 decoder's training pass with bf16-operand dense layers (`matmul="bf16"`), in
any dtype: tests/gpt2_dropout_ref.py without dropout, where every dense projection -- c_attn, attn.c_proj, c_fc,
mlp.c_proj and the tied lm_head -- is ONE autograd function that rounds both operands of each of its three products to
bf16: x and W in the forward, dy and W for dx, x and dy for dW.  Sums, biases, the bias gradient and everything between
the dense layers stay in the working dtype.  `rnd=False` switches the rounding off: the function is then a plain dense
layer and `run` equals `gpt2_dropout_ref.run` without masks.

`round_bf16` rounds to nearest, ties to even, by integer arithmetic on the fp32 bit pattern (its own statement of the
rule, not torch's cast); fp64 values pass through fp32 first, as the kernel's operands are fp32 in memory."""
import torch
import torch.nn.functional as F

import gpt2_dropout_ref as gref


def round_bf16(t):
    """t rounded to the nearest bf16 (ties to even), returned in t's dtype.  Finite inputs only."""
    u = t.detach().float().contiguous().view(torch.int32)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & -65536
    return u.view(torch.float32).to(t.dtype)


class DenseBf16(torch.autograd.Function):
    """y = r(x) r(W) + b for x [..., in], W [in, out]; dx = r(dy) r(W)^T, dW = r(x)^T r(dy), db = sum dy."""

    @staticmethod
    def forward(ctx, x, w, b, rnd):
        r = round_bf16 if rnd else (lambda v: v)
        ctx.save_for_backward(x, w)
        ctx.r, ctx.has_b = r, b is not None
        y = r(x) @ r(w)
        return y if b is None else y + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        r = ctx.r
        x2, dy2 = x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])
        dx = (r(dy2) @ r(w).t()).view(x.shape)
        dw = r(x2).t() @ r(dy2)
        return dx, dw, dy2.sum(0) if ctx.has_b else None, None


def forward(w, tokens, key_mask, n_layer, n_head, rnd=True):
    """w: {huggingface name: tensor} in the working dtype -> logits [R, L, V]."""
    wte, wpe = w["transformer.wte.weight"], w["transformer.wpe.weight"]
    r, l = tokens.shape
    d = wte.shape[1]

    def dense(x, name):
        return DenseBf16.apply(x, w[name + ".weight"], w[name + ".bias"], rnd)

    h = wte[tokens] + wpe[torch.arange(l)][None]
    for i in range(n_layer):
        q = f"transformer.h.{i}."
        a = F.layer_norm(h, (d,), w[q + "ln_1.weight"], w[q + "ln_1.bias"], 1e-5)
        qkv = dense(a, q + "attn.c_attn")
        o = gref.attention(qkv.reshape(r * l, 3 * d), key_mask, r, l, n_head, d // n_head)
        h = h + dense(o.view(r, l, d), q + "attn.c_proj")
        m = F.layer_norm(h, (d,), w[q + "ln_2.weight"], w[q + "ln_2.bias"], 1e-5)
        f = gref.gelu_new(dense(m, q + "mlp.c_fc"))
        h = h + dense(f, q + "mlp.c_proj")
    hf = F.layer_norm(h, (d,), w["transformer.ln_f.weight"], w["transformer.ln_f.bias"], 1e-5)
    return DenseBf16.apply(hf, wte.t(), None, rnd)


def run(weights, tokens, key_mask, n_layer, n_head, pad, label_sets, dtype, rnd=True):
    """-> logits, the losses of every label set (a vector), the gradients of the first loss {name: tensor}."""
    w = {k: v.to(dtype).clone().requires_grad_(True) for k, v in weights.items()}
    logits = forward(w, tokens, key_mask, n_layer, n_head, rnd)
    losses = torch.stack([gref.lm_loss(logits, lb, pad) for lb in label_sets])
    names = list(w)
    grads = torch.autograd.grad(losses[0], [w[k] for k in names])
    return logits.detach(), losses.detach(), dict(zip(names, grads))
