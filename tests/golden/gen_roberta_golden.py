"""Generates tests/golden/roberta_*.npz with the INSTALLED huggingface transformers RobertaModel /
RobertaForSequenceClassification (the third-party code `vidsitu_code/mdl_evrel.py:21,62` calls; the reference pins
transformers==3.3.1, this container has a newer release of the same published model) in fp64, on the weights of
tests/roberta_ref.make_weights(seed).  Run from the repo root: python tests/golden/gen_roberta_golden.py

Cases (right-padded batches, every row with at least three valid tokens; a row whose mask is all zero is treated
differently by newer releases and is kept out of the goldens):
  tiny  2 layers, 64 wide, 6 x 60: tokens, mask, every hidden state, pooler output, logits, and -- in a file of its own --
        the 5-label cross-entropy loss of the classification model with every parameter gradient;
  wide  a 2-layer slice of roberta-base's shape (768 wide, 12 heads) at 3 x 120: every second position of the last
        hidden state (the whole of it would pass the size limit for committed files), pooler output, logits.
The weights are re-derived from the seed by the tests.
Also writes evrel_state_dict_names.json: the state-dict keys of the reference's five event-relation models, read off
huggingface's own modules (2-layer encoder) beside the reference's three `nn.Sequential(Linear, ReLU, Linear)` heads
(`mdl_evrel.py:21-23,62-76`)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import roberta_ref as ref  # noqa: E402
from transformers import RobertaConfig, RobertaForSequenceClassification, RobertaModel  # noqa: E402

CASES = [("tiny", ref.TINY, 6, 60, 21), ("wide", ref.WIDE, 3, 120, 22)]


def hf_config(dims):
    return RobertaConfig(vocab_size=dims["vocab_size"], hidden_size=dims["d_model"],
                         num_hidden_layers=dims["n_layer"], num_attention_heads=dims["n_head"],
                         intermediate_size=dims["d_ffn"], max_position_embeddings=dims["n_positions"],
                         type_vocab_size=1, pad_token_id=dims["pad_token_id"], bos_token_id=0, eos_token_id=2,
                         layer_norm_eps=dims["layer_norm_eps"], hidden_dropout_prob=0.0,
                         attention_probs_dropout_prob=0.0, hidden_act="gelu", num_labels=5,
                         attn_implementation="eager")


def load(model, w):
    missing, unexpected = model.load_state_dict(w, strict=False)
    assert not unexpected and all(k.endswith("position_ids") or k.endswith("token_type_ids") for k in missing), \
        (missing, unexpected)


for name, dims, R, L, seed in CASES:
    toks, mask = ref.golden_inputs(dims, R, L, seed + 100)
    w = ref.make_weights(dims, seed)  # encoder + pooler
    wc = ref.make_weights(dims, seed, prefix="roberta.", pooler=False, num_labels=5)  # same encoder, + head
    for k in w:
        if not k.startswith("pooler."):
            assert torch.equal(w[k], wc["roberta." + k])
    m = RobertaModel(hf_config(dims), add_pooling_layer=True).double().eval()
    load(m, w)
    mc = RobertaForSequenceClassification(hf_config(dims)).double().eval()
    load(mc, wc)
    with torch.no_grad():
        out = m(input_ids=toks, attention_mask=mask, output_hidden_states=True)
        logits = mc(input_ids=toks, attention_mask=mask).logits
    hs = ref.encoder(w, toks, mask, dims, all_hidden=True)
    err_h = max(float((a - b).abs().max()) for a, b in zip(hs, out.hidden_states))
    err_p = float((ref.pooler(w, hs[-1]) - out.pooler_output).abs().max())
    err_l = float((ref.classifier(wc, ref.encoder(wc, toks, mask, dims, prefix="roberta.")) - logits).abs().max())
    print(f"{name}: |restatement - HF| hidden {err_h:.3e} pooler {err_p:.3e} logits {err_l:.3e}")
    store = {"tokens": toks.numpy(), "mask": mask.numpy(), "pooler_output": out.pooler_output.numpy(),
             "logits": logits.numpy()}
    if name == "tiny":
        store["hidden_states"] = torch.stack(list(out.hidden_states)).numpy()
        g = torch.Generator(device="cpu").manual_seed(seed + 200)
        labels = torch.randint(0, 5, (R,), generator=g)
        mc.zero_grad()
        loss = torch.nn.functional.cross_entropy(mc(input_ids=toks, attention_mask=mask).logits, labels)
        loss.backward()
        grads = {"grad." + k: v.grad.numpy().copy() for k, v in mc.named_parameters()}
        grads["loss"] = np.float64(loss.item())
        grads["labels"] = labels.numpy()
        wl = {k: v.clone().requires_grad_(True) for k, v in wc.items()}
        rl = torch.nn.functional.cross_entropy(
            ref.classifier(wl, ref.encoder(wl, toks, mask, dims, prefix="roberta.")), labels)
        rl.backward()
        gmax = max(float(np.abs(v).max()) for k, v in grads.items() if k.startswith("grad."))
        gerr = max(float((wl[k[5:]].grad - torch.from_numpy(v)).abs().max()) for k, v in grads.items()
                   if k.startswith("grad."))
        print(f"{name}: loss {loss.item():.6f} (restatement {rl.item():.6f}), gradient error {gerr:.3e} on the scale "
              f"{gmax:.3e}")
        np.savez_compressed(os.path.join(HERE, "roberta_tiny_grads.npz"), **grads)
    else:
        store["last_hidden_even"] = out.last_hidden_state[:, ::2].numpy().astype(np.float32)
    np.savez_compressed(os.path.join(HERE, f"roberta_{name}.npz"), **store)
    print(f"{name}: wrote", {k: v.shape for k, v in store.items()})


def _persistent(model):
    return [k for k in model.state_dict() if not k.endswith("position_ids") and not k.endswith("token_type_ids")]


heads = torch.nn.ModuleDict({
    "vid_feat_encoder": torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.ReLU(), torch.nn.Linear(8, 8)),
    "vis_lang_encoder": torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.ReLU(), torch.nn.Linear(8, 8)),
    "vis_lang_classf": torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.ReLU(), torch.nn.Linear(8, 5))})
with_pooler = ["rob_mdl." + k for k in _persistent(RobertaModel(hf_config(ref.TINY), add_pooling_layer=True))] \
    + list(heads.state_dict())
names = {"rob_evrel": ["rob_mdl." + k for k in _persistent(RobertaForSequenceClassification(hf_config(ref.TINY)))]}
for row in ("txe_evrel", "sfpret_evrel", "sfpret_vbonly_evrel", "sfpret_onlyvid_evrel"):
    names[row] = with_pooler
with open(os.path.join(HERE, "evrel_state_dict_names.json"), "w") as f:
    json.dump(names, f, indent=0)
print("state-dict names:", {k: len(v) for k, v in names.items()})
