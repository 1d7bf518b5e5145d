"""Plain torch restatement of the GPT-2 decoder's training pass with dropout as MASK OPERANDS, in any dtype (fp64
reference, fp32 noise floor): transformers 3.3.1 modeling_gpt2 applies dropout in four places -- on the summed
embeddings, on the attention probabilities after the softmax, after attn.c_proj and after mlp.c_proj (both before
the residual add).  Sites: 0 = embedding, 1 + 3i / 2 + 3i / 3 + 3i = those three of layer i.  The masks come from
tests/dropout_ref.py; autograd differentiates through them."""
import math

import torch
import torch.nn.functional as F

import dropout_ref

GELU_K, GELU_C = math.sqrt(2.0 / math.pi), 0.044715


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(GELU_K * (x + GELU_C * x * x * x)))


def masks(seed, step, n_layer, r, l, d, n_head, p_embd, p_attn, p_resid):
    """{site: fp64 tensor of 0 / scale} for every site whose probability is above 0 (scale as the host rounds it)."""
    out = {}

    def flat(site, p):
        thr, scale = dropout_ref.threshold(p)
        out[site] = torch.from_numpy(dropout_ref.keep_flat(seed, step, site, r * l * d, thr)).double().view(r, l, d) * scale

    if p_embd > 0:
        flat(0, p_embd)
    for i in range(n_layer):
        if p_attn > 0:
            thr, scale = dropout_ref.threshold(p_attn)
            out[1 + 3 * i] = torch.from_numpy(dropout_ref.keep_attn(seed, step, 1 + 3 * i, r, n_head, l, thr)).double() * scale
        if p_resid > 0:
            flat(2 + 3 * i, p_resid)
            flat(3 + 3 * i, p_resid)
    return out


def attention(qkv, key_mask, r, l, h, dh, drop=None):
    """modeling_gpt2 Attention._attn on the fused projection [R*L, 3D]; drop [R, H, L, L] multiplies the
    probabilities.  No query of the callers' inputs is fully masked unless its upstream gradient is zero."""
    dt = qkv.dtype
    x = qkv.view(r, l, 3, h, dh)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    causal = torch.ones(l, l, dtype=torch.bool).tril()
    s = torch.where(causal, s, torch.full((), -1e4, dtype=dt))
    if key_mask is not None:
        s = s + (1.0 - key_mask.to(dt))[:, None, None, :] * -1e4
    p = torch.softmax(s, -1)
    if drop is not None:
        p = p * drop.to(dt)
    return (p @ v).transpose(1, 2).reshape(r * l, h * dh)


def forward(w, tokens, key_mask, n_layer, n_head, drops):
    """w: {huggingface name: tensor} in the working dtype -> logits [R, L, V]."""
    wte, wpe = w["transformer.wte.weight"], w["transformer.wpe.weight"]
    dt = wte.dtype
    r, l = tokens.shape
    d = wte.shape[1]

    def drop(x, site):
        return x * drops[site].to(dt).view(x.shape) if site in drops else x

    h = drop(wte[tokens] + wpe[torch.arange(l)][None], 0)
    for i in range(n_layer):
        q = f"transformer.h.{i}."
        a = F.layer_norm(h, (d,), w[q + "ln_1.weight"], w[q + "ln_1.bias"], 1e-5)
        qkv = a @ w[q + "attn.c_attn.weight"] + w[q + "attn.c_attn.bias"]
        o = attention(qkv.reshape(r * l, 3 * d), key_mask, r, l, n_head, d // n_head, drops.get(1 + 3 * i))
        h = h + drop(o.view(r, l, d) @ w[q + "attn.c_proj.weight"] + w[q + "attn.c_proj.bias"], 2 + 3 * i)
        m = F.layer_norm(h, (d,), w[q + "ln_2.weight"], w[q + "ln_2.bias"], 1e-5)
        f = gelu_new(m @ w[q + "mlp.c_fc.weight"] + w[q + "mlp.c_fc.bias"])
        h = h + drop(f @ w[q + "mlp.c_proj.weight"] + w[q + "mlp.c_proj.bias"], 3 + 3 * i)
    hf = F.layer_norm(h, (d,), w["transformer.ln_f.weight"], w["transformer.ln_f.bias"], 1e-5)
    return hf @ wte.t()


def lm_loss(logits, labels_from, pad):
    """CE(logits[:, :-1], labels_from[:, 1:]), ignore_index = pad, mean over the counted tokens."""
    v = logits.shape[-1]
    return F.cross_entropy(logits[:, :-1].reshape(-1, v), labels_from[:, 1:].reshape(-1), ignore_index=pad)


def run(weights, tokens, key_mask, n_layer, n_head, drops, pad, label_sets, dtype):
    """-> logits, the losses of every label set (a vector), the gradients of the first loss {name: tensor}."""
    w = {k: v.to(dtype).clone().requires_grad_(True) for k, v in weights.items()}
    logits = forward(w, tokens, key_mask, n_layer, n_head, drops)
    losses = torch.stack([lm_loss(logits, lb, pad) for lb in label_sets])
    names = list(w)
    grads = torch.autograd.grad(losses[0], [w[k] for k in names])
    return logits.detach(), losses.detach(), dict(zip(names, grads))
