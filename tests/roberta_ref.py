"""Plain-torch restatement of the RoBERTa encoder, its pooler, the classification head and the five event-relation
models (`vidsitu_code/mdl_evrel.py`), dtype-generic (fp64 is the yardstick of the GPU tests, fp32 gives the
restatement's own rounding error).  Rules of the pinned transformers release (3.3.1):

  * additive key mask (1 - attention_mask) * -1e4 on the scaled scores, softmax over all keys;
  * position ids from the token ids: cumsum(tok != pad) * (tok != pad) + pad;
  * one token-type row; post-LN residual blocks; erf GELU; LayerNorm eps 1e-5;
  * pooler tanh(dense(h[:, 0])); classification head out_proj(tanh(dense(h[:, 0]))); no dropout.

Weights are a dict under huggingface's parameter names; `make_weights` / `make_evrel_weights` derive them from a seed.
"""
import math

import torch

TINY = dict(n_layer=2, d_model=64, n_head=2, n_positions=130, vocab_size=101, d_ffn=128, pad_token_id=1,
            layer_norm_eps=1e-5)
WIDE = dict(n_layer=2, d_model=768, n_head=12, n_positions=130, vocab_size=211, d_ffn=3072, pad_token_id=1,
            layer_norm_eps=1e-5)  # a 2-layer slice of roberta-base's shape
EVREL_NAMES = ("rob_evrel", "txe_evrel", "sfpret_evrel", "sfpret_vbonly_evrel", "sfpret_onlyvid_evrel")
EV_FIRST, EV_SECOND = [0, 1, 2, 2], [2, 2, 3, 4]


def encoder_names(dims, prefix="", pooler=True):
    names = [prefix + "embeddings.word_embeddings.weight", prefix + "embeddings.position_embeddings.weight",
             prefix + "embeddings.token_type_embeddings.weight", prefix + "embeddings.LayerNorm.weight",
             prefix + "embeddings.LayerNorm.bias"]
    for i in range(dims["n_layer"]):
        q = f"{prefix}encoder.layer.{i}."
        for m in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
                  "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm"):
            names += [q + m + ".weight", q + m + ".bias"]
    if pooler:
        names += [prefix + "pooler.dense.weight", prefix + "pooler.dense.bias"]
    return names


def _shape(name, dims, num_labels):
    d, f = dims["d_model"], dims["d_ffn"]
    leaf = name.rsplit(".", 1)[0]
    is_w = name.endswith(".weight")
    if "word_embeddings" in name:
        return (dims["vocab_size"], d)
    if "position_embeddings" in name:
        return (dims["n_positions"], d)
    if "token_type_embeddings" in name:
        return (1, d)
    if "LayerNorm" in name:
        return (d,)
    if leaf.endswith("intermediate.dense"):
        return (f, d) if is_w else (f,)
    if leaf.endswith("output.dense") and "attention" not in leaf:
        return (d, f) if is_w else (d,)
    if leaf.endswith("classifier.out_proj"):
        return (num_labels, d) if is_w else (num_labels,)
    return (d, d) if is_w else (d,)


def make_weights(dims, seed, prefix="", pooler=True, num_labels=0, dtype=torch.float64):
    """Seeded weights with every parameter away from its initial value (LayerNorm gains around 1, biases not zero,
    padding rows of the embedding tables not zero: a loaded checkpoint's are not either)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    names = encoder_names(dims, prefix, pooler)
    if num_labels:
        names += ["classifier.dense.weight", "classifier.dense.bias", "classifier.out_proj.weight",
                  "classifier.out_proj.bias"]
    w = {}
    for n in names:
        shp = _shape(n, dims, num_labels)
        t = torch.randn(*shp, generator=g, dtype=torch.float64)
        if "LayerNorm.weight" in n:
            t = 1.0 + 0.1 * t
        elif n.endswith(".bias"):
            t = 0.05 * t
        elif "embeddings" in n:
            t = 0.5 * t
        else:
            t = t * (1.5 / math.sqrt(shp[1]))
        w[n] = t.to(dtype)
    return w


def position_ids(tokens, pad):
    m = tokens.ne(pad).long()
    return torch.cumsum(m, dim=1) * m + pad


def layer_norm(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention(qkv, mask, n_head):
    """qkv [R, L, 3D], mask [R, L] {0,1} or None -> [R, L, D] (the kernel's contract, vs_attn_pad_fwd)."""
    r, l, d3 = qkv.shape
    d = d3 // 3
    dh = d // n_head
    q, k, v = (t.reshape(r, l, n_head, dh).transpose(1, 2) for t in qkv.split(d, dim=-1))
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    if mask is not None:
        s = s + (1.0 - mask.to(qkv.dtype))[:, None, None, :] * -1e4
    p = torch.softmax(s, dim=-1)
    return (p @ v).transpose(1, 2).reshape(r, l, d)


def embed(w, tokens, dims, prefix=""):
    pid = position_ids(tokens, dims["pad_token_id"])
    e = w[prefix + "embeddings.word_embeddings.weight"][tokens] \
        + w[prefix + "embeddings.position_embeddings.weight"][pid] \
        + w[prefix + "embeddings.token_type_embeddings.weight"][0]
    return e, pid


def encoder(w, tokens, mask, dims, prefix="", all_hidden=False):
    """-> last hidden state [R, L, D] (or the list of all n_layer + 1 hidden states)."""
    eps, nh = dims["layer_norm_eps"], dims["n_head"]

    def lin(x, name):
        return x @ w[prefix + name + ".weight"].t() + w[prefix + name + ".bias"]

    def ln(x, name):
        return layer_norm(x, w[prefix + name + ".weight"], w[prefix + name + ".bias"], eps)

    e, _ = embed(w, tokens, dims, prefix)
    h = ln(e, "embeddings.LayerNorm")
    hs = [h]
    for i in range(dims["n_layer"]):
        q = f"encoder.layer.{i}."
        qkv = torch.cat([lin(h, q + "attention.self." + s) for s in ("query", "key", "value")], dim=-1)
        ctx = attention(qkv, mask, nh)
        h = ln(lin(ctx, q + "attention.output.dense") + h, q + "attention.output.LayerNorm")
        f = gelu(lin(h, q + "intermediate.dense"))
        h = ln(lin(f, q + "output.dense") + h, q + "output.LayerNorm")
        hs.append(h)
    return hs if all_hidden else h


def pooler(w, h, prefix=""):
    return torch.tanh(h[:, 0] @ w[prefix + "pooler.dense.weight"].t() + w[prefix + "pooler.dense.bias"])


def classifier(w, h):
    c = torch.tanh(h[:, 0] @ w["classifier.dense.weight"].t() + w["classifier.dense.bias"])
    return c @ w["classifier.out_proj.weight"].t() + w["classifier.out_proj.bias"]


# ---- the five event-relation models -----------------------------------------------------------------------------
def evrel_state_names(name, dims):
    """State-dict keys of the model behind selector row `name`, in registration order."""
    if name == "rob_evrel":
        return ["rob_mdl." + n for n in encoder_names(dims, "roberta.", pooler=False)] + \
            ["rob_mdl.classifier.dense.weight", "rob_mdl.classifier.dense.bias", "rob_mdl.classifier.out_proj.weight",
             "rob_mdl.classifier.out_proj.bias"]
    names = ["rob_mdl." + n for n in encoder_names(dims, "", pooler=True)]
    for m in ("vid_feat_encoder", "vis_lang_encoder", "vis_lang_classf"):
        names += [f"{m}.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")]
    return names


def make_evrel_weights(name, dims, head_dim, seed, dtype=torch.float64):
    if name == "rob_evrel":
        w = make_weights(dims, seed, prefix="roberta.", pooler=False, num_labels=5, dtype=dtype)
        return {"rob_mdl." + k: v for k, v in w.items()}
    w = {"rob_mdl." + k: v for k, v in make_weights(dims, seed, dtype=dtype).items()}
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    d = dims["d_model"]
    for m, sizes in (("vid_feat_encoder", ((1024, head_dim), (1024, 1024))),
                     ("vis_lang_encoder", ((1024, 1024 + d), (1024, 1024))),
                     ("vis_lang_classf", ((1024, 2048), (5, 1024)))):
        for i, (n_out, n_in) in zip((0, 2), sizes):
            w[f"{m}.{i}.weight"] = (torch.randn(n_out, n_in, generator=g, dtype=torch.float64)
                                    * (1.5 / math.sqrt(n_in))).to(dtype)
            w[f"{m}.{i}.bias"] = (0.05 * torch.randn(n_out, generator=g, dtype=torch.float64)).to(dtype)
    return w


def _mlp(w, m, x):
    h = torch.relu(x @ w[m + ".0.weight"].t() + w[m + ".0.bias"])
    return h @ w[m + ".2.weight"].t() + w[m + ".2.bias"]


def evrel_forward(name, w, batch, dims):
    """-> (mdl_out [B, 4, n_ann, 5], loss): the reference's forward, branches it multiplies out included as zeros."""
    dtype = w["rob_mdl." + ("roberta." if name == "rob_evrel" else "") + "embeddings.LayerNorm.weight"].dtype
    labels = batch["evrel_labs"].reshape(-1)
    if name == "rob_evrel":
        toks, mask = batch["evrel_seq_out"], batch["evrel_seq_out_lens"]
        b, ne, na, l = toks.shape
        sub = {k[len("rob_mdl."):]: v for k, v in w.items()}
        h = encoder(sub, toks.reshape(-1, l), mask.reshape(-1, l), dims, prefix="roberta.")
        logits = classifier(sub, h)
        loss = torch.nn.functional.cross_entropy(logits, labels)
        return logits.view(b, ne, na, 5), loss
    key = "evrel_vbonly_out_ones" if name == "sfpret_vbonly_evrel" else "evrel_seq_out_ones"
    toks, mask = batch[key], batch[key + "_lens"]
    b, ne, na, l = toks.shape
    sub = {k[len("rob_mdl."):]: v for k, v in w.items() if k.startswith("rob_mdl.")}
    pooled = pooler(sub, encoder(sub, toks.reshape(-1, l), mask.reshape(-1, l), dims)).view(b, 5, na, -1)
    vis = _mlp(w, "vid_feat_encoder", batch["frm_feats"].to(dtype)).view(b, 5, 1, -1).expand(b, 5, na, -1)
    if name == "sfpret_onlyvid_evrel":
        pooled = torch.zeros_like(pooled)
    if name == "txe_evrel":
        vis = torch.zeros_like(vis)
    vl = _mlp(w, "vis_lang_encoder", torch.cat([vis, pooled], dim=-1))
    pair = torch.cat([vl[:, EV_FIRST], vl[:, EV_SECOND]], dim=-1)
    logits = _mlp(w, "vis_lang_classf", pair)
    loss = torch.nn.functional.cross_entropy(logits.reshape(-1, 5), labels)
    return logits.view(b, ne - 1, na, 5), loss


def evrel_loss_and_grads(name, w, batch, dims):
    """-> (mdl_out, loss, {name: grad | None}) with autograd on a copy of the weights."""
    wl = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    out, loss = evrel_forward(name, wl, batch, dims)
    loss.backward()
    return out.detach(), loss.detach(), {k: v.grad for k, v in wl.items()}


def golden_inputs(dims, r, l, seed):
    """Right-padded token batch of the goldens: row 0 full, the others shorter, the last one 3 tokens long."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    pad = dims["pad_token_id"]
    toks = torch.randint(4, dims["vocab_size"], (r, l), generator=g)
    mask = torch.ones((r, l), dtype=torch.long)
    for i in range(1, r):
        n = 3 if i == r - 1 else l - (i * 11) % (l - 4)
        toks[i, n:] = pad
        mask[i, n:] = 0
    toks[:, 0] = 0
    for i in range(r):
        toks[i, int(mask[i].sum()) - 1] = 2
    return toks, mask
