"""CPU checks of the event-relation task: the plain-torch restatement (tests/roberta_ref.py) against goldens made with
huggingface transformers (tests/golden/gen_roberta_golden.py), the selector's five rows, the models' state-dict keys
against the committed list, and the synthetic batch contract.  No GPU, no transformers import."""
import json
import os

import numpy as np
import pytest
import torch

import roberta_ref as ref
from vidsitu_amd import synth_data
from vidsitu_amd.extended_config import get_cfg
from vidsitu_amd.mdl_selector import get_mdl_loss_eval

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gold(name):
    return {k: v for k, v in np.load(os.path.join(GOLD, name)).items()}


def _cfg(row):
    return get_cfg({"task_type": "evrel", "mdl.mdl_name": row, "mdl.rob_mdl_name": "roberta-synth-tiny"})


def test_restatement_matches_the_tiny_golden():
    g = _gold("roberta_tiny.npz")
    toks, mask = torch.from_numpy(g["tokens"]), torch.from_numpy(g["mask"])
    w = ref.make_weights(ref.TINY, 21)
    hs = ref.encoder(w, toks, mask, ref.TINY, all_hidden=True)
    assert len(hs) == g["hidden_states"].shape[0] == 3
    for i, h in enumerate(hs):
        assert float((h - torch.from_numpy(g["hidden_states"][i])).abs().max()) < 1e-12, f"hidden state {i}"
    assert float((ref.pooler(w, hs[-1]) - torch.from_numpy(g["pooler_output"])).abs().max()) < 1e-12
    wc = ref.make_weights(ref.TINY, 21, prefix="roberta.", pooler=False, num_labels=5)
    logits = ref.classifier(wc, ref.encoder(wc, toks, mask, ref.TINY, prefix="roberta."))
    assert float((logits - torch.from_numpy(g["logits"])).abs().max()) < 1e-12


def test_restatement_matches_the_tiny_golden_gradients():
    g, gg = _gold("roberta_tiny.npz"), _gold("roberta_tiny_grads.npz")
    toks, mask = torch.from_numpy(g["tokens"]), torch.from_numpy(g["mask"])
    wc = {k: v.requires_grad_(True) for k, v in
          ref.make_weights(ref.TINY, 21, prefix="roberta.", pooler=False, num_labels=5).items()}
    loss = torch.nn.functional.cross_entropy(
        ref.classifier(wc, ref.encoder(wc, toks, mask, ref.TINY, prefix="roberta.")), torch.from_numpy(gg["labels"]))
    loss.backward()
    assert abs(float(loss.detach()) - float(gg["loss"])) < 1e-12
    names = [k[5:] for k in gg if k.startswith("grad.")]
    assert sorted(names) == sorted(wc)
    # key.bias gradients are analytically zero (rounding noise in both): every gradient is compared on the absolute
    # scale of the largest one, never relative to itself
    scale = max(float(np.abs(gg["grad." + k]).max()) for k in names)
    for k in names:
        err = float((wc[k].grad - torch.from_numpy(gg["grad." + k])).abs().max())
        assert err < 1e-12 * scale, f"{k}: {err:.3e} on the scale {scale:.3e}"
    kb = float(np.abs(gg["grad.roberta.encoder.layer.0.attention.self.key.bias"]).max())
    assert kb < 1e-12 * scale
    pad = ref.TINY["pad_token_id"]
    assert float(np.abs(gg["grad.roberta.embeddings.word_embeddings.weight"][pad]).max()) == 0.0
    assert float(np.abs(gg["grad.roberta.embeddings.position_embeddings.weight"][pad]).max()) == 0.0


def test_restatement_matches_the_wide_golden():
    g = _gold("roberta_wide.npz")
    toks, mask = torch.from_numpy(g["tokens"]), torch.from_numpy(g["mask"])
    w = ref.make_weights(ref.WIDE, 22)
    h = ref.encoder(w, toks, mask, ref.WIDE)
    stored = torch.from_numpy(g["last_hidden_even"]).double()  # kept in fp32: half an ulp of the largest entry
    assert float((h[:, ::2] - stored).abs().max()) <= 2.0 ** -24 * float(stored.abs().max()) * 1.01
    assert float((ref.pooler(w, h) - torch.from_numpy(g["pooler_output"])).abs().max()) < 1e-12
    wc = ref.make_weights(ref.WIDE, 22, prefix="roberta.", pooler=False, num_labels=5)
    logits = ref.classifier(wc, ref.encoder(wc, toks, mask, ref.WIDE, prefix="roberta."))
    assert float((logits - torch.from_numpy(g["logits"])).abs().max()) < 1e-12


def test_all_zero_mask_row_equals_the_unmasked_row():
    """Under the additive -1e4 rule a sequence whose mask is all zero attends as if nothing were masked (newer
    huggingface releases treat it differently: this case stays out of the goldens)."""
    g = _gold("roberta_tiny.npz")
    toks, mask = torch.from_numpy(g["tokens"]), torch.from_numpy(g["mask"]).clone()
    w = ref.make_weights(ref.TINY, 21)
    zero, full = mask.clone(), mask.clone()
    zero[2], full[2] = 0, 1
    hz, hf = ref.encoder(w, toks, zero, ref.TINY), ref.encoder(w, toks, full, ref.TINY)
    assert float((hz[2] - hf[2]).abs().max()) < 1e-9  # (scores near 1e4 keep about 1e-12 of absolute precision)
    assert float((hz[0] - hf[0]).abs().max()) == 0.0


def test_position_ids_come_from_the_token_ids():
    toks = torch.tensor([[0, 7, 1, 9, 2, 1, 1], [1, 1, 0, 5, 2, 1, 8]])
    assert ref.position_ids(toks, 1).tolist() == [[2, 3, 1, 4, 5, 1, 1], [1, 1, 2, 3, 4, 1, 5]]


@pytest.mark.parametrize("row", ref.EVREL_NAMES)
def test_selector_returns_the_evrel_rows(row):
    from vidsitu_amd import evl_vsitu, mdl_evrel, mdl_sf_base

    want = {"rob_evrel": mdl_evrel.Simple_EvRel_Roberta, "txe_evrel": mdl_evrel.Simple_TxEncEvRel,
            "sfpret_evrel": mdl_evrel.SFPret_SimpleEvRel, "sfpret_vbonly_evrel": mdl_evrel.SFPret_OnlyVb_SimpleEvRel,
            "sfpret_onlyvid_evrel": mdl_evrel.SFPret_OnlyVid_SimpleEvRel}
    sel = get_mdl_loss_eval(_cfg(row))
    assert sel["mdl"] is want[row] and sel["loss"] is mdl_sf_base.LossLambda and sel["evl"] is evl_vsitu.EvalB_Acc


def test_selector_still_refuses_unknown_evrel_names():
    cfg = get_cfg({"task_type": "evrel", "mdl.mdl_name": "sf_base"})
    with pytest.raises(NotImplementedError):
        get_mdl_loss_eval(cfg)


@pytest.mark.parametrize("row", ref.EVREL_NAMES)
def test_state_dict_names_match_the_committed_list(row):
    with open(os.path.join(GOLD, "evrel_state_dict_names.json")) as f:
        committed = json.load(f)[row]
    cfg = _cfg(row)
    mdl = get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=synth_data.make_comm(cfg))
    sd = mdl.state_dict()
    assert sorted(sd) == sorted(committed)
    from vidsitu_amd.hf_roberta import ROBERTA_DIMS

    dims = ROBERTA_DIMS["roberta-synth-tiny"]
    assert sorted(sd) == sorted(ref.evrel_state_names(row, dims))
    if row != "rob_evrel":
        assert tuple(sd["vis_lang_encoder.0.weight"].shape) == (1024, 1024 + dims["d_model"])
        assert tuple(sd["vis_lang_classf.2.weight"].shape) == (5, 1024)
    # a checkpoint of the pinned release also carries the position-id buffer: ignored, nothing else is
    sd2 = dict(sd)
    pre = "rob_mdl.roberta." if row == "rob_evrel" else "rob_mdl."
    sd2[pre + "embeddings.position_ids"] = torch.arange(dims["n_positions"]).unsqueeze(0)
    assert mdl.load_state_dict(sd2, strict=True)
    sd2["rob_mdl.not_a_parameter"] = torch.zeros(1)
    with pytest.raises(RuntimeError):
        mdl.load_state_dict(sd2, strict=True)


def test_roberta_base_dimensions():
    from vidsitu_amd.hf_roberta import ROBERTA_DIMS

    d = ROBERTA_DIMS["roberta-base"]
    assert (d["n_layer"], d["d_model"], d["n_head"], d["n_positions"], d["vocab_size"], d["d_ffn"],
            d["pad_token_id"], d["layer_norm_eps"]) == (12, 768, 12, 514, 50265, 3072, 1, 1e-5)


@pytest.mark.parametrize("n_ann", [1, 3])
def test_synth_evrel_batch_contract(n_ann):
    cfg = _cfg("sfpret_evrel")
    comm = synth_data.make_comm(cfg)
    assert comm.evrel_dct == {"Null": 0, "Causes": 1, "Reaction To": 2, "Enables": 3, "NoRel": 4}
    assert comm.evrel_dct_opp[2] == "Reaction To" and comm.rob_hf_tok.pad_token_id == 1
    b = synth_data.synth_evrel_batch(comm, 3, n_ann=n_ann, feat_dim=2304, seed=5)
    for key, shape in (("evrel_seq_out", (3, 4, n_ann, 120)), ("evrel_seq_out_ones", (3, 5, n_ann, 60)),
                       ("evrel_vbonly_out_ones", (3, 5, n_ann, 5))):
        seq, mask = b[key], b[key + "_lens"]
        assert tuple(seq.shape) == shape == tuple(mask.shape) and seq.dtype == mask.dtype == torch.int64
        assert int(seq.max()) < len(comm.rob_hf_tok) and int(seq.min()) >= 0
        flat_s, flat_m = seq.view(-1, shape[-1]), mask.view(-1, shape[-1])
        n = flat_m.sum(1)
        assert bool((n >= 3).all()) and bool((flat_s[:, 0] == 0).all())
        for s, m, k in zip(flat_s, flat_m, n.tolist()):
            assert m[:k].all() and not m[k:].any()          # right padding
            assert int(s[k - 1]) == 2 and bool((s[k:] == 1).all()) and not bool((s[:k] == 1).any())
    assert tuple(b["evrel_labs"].shape) == (3, 4, n_ann) and 0 <= int(b["evrel_labs"].min()) \
        and int(b["evrel_labs"].max()) <= 4
    assert tuple(b["frm_feats"].shape) == (3, 5, 2304) and b["vseg_idx"].tolist() == [0, 1, 2]
    again = synth_data.synth_evrel_batch(comm, 3, n_ann=n_ann, feat_dim=2304, seed=5)
    assert all(torch.equal(b[k], again[k]) for k in b)


def test_evrel_restatement_skipped_branches_have_no_gradient():
    """What the reference multiplies out of the result has no gradient in the restatement either."""
    cfg = _cfg("txe_evrel")
    comm = synth_data.make_comm(cfg)
    batch = synth_data.synth_evrel_batch(comm, 2, n_ann=1, feat_dim=32, seed=3)
    dims = dict(ref.TINY)
    for row, dead in (("txe_evrel", "vid_feat_encoder."), ("sfpret_onlyvid_evrel", "rob_mdl.")):
        w = ref.make_evrel_weights(row, dims, 32, 7)
        out, loss, grads = ref.evrel_loss_and_grads(row, w, batch, dims)
        assert tuple(out.shape) == (2, 4, 1, 5) and float(loss) > 0
        for k, g in grads.items():
            if k.startswith(dead):
                assert g is None or float(g.abs().max()) == 0.0, k
            else:
                assert g is not None, k
