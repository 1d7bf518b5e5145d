"""CPU side of the RoBERTa dropout: the restatement (tests/roberta_dropout_ref.py) against roberta_ref, the site
numbering, the config key, the C ABI's new symbols and the host logic that needs no GPU."""
import os
import re

import pytest
import torch

import dropout_ref
import roberta_dropout_ref as dref
import roberta_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vs_attn_pad_drop_fwd", "vs_attn_pad_drop_bwd")
SEED = (0x51ed << 32) | 0x2705a3c9


def _inputs():
    toks, mask = ref.golden_inputs(ref.TINY, 3, 17, 9)
    return toks, mask


def test_every_probability_zero_is_roberta_ref_exactly():
    toks, mask = _inputs()
    n = ref.TINY["n_layer"]
    for dt in (torch.float64, torch.float32):
        w = ref.make_weights(ref.TINY, 3, dtype=dt)
        drops = dref.masks(SEED, 4, ref.TINY, 3, 17, 0.0, 0.0)
        assert all(v is None for v in drops.values())
        for dr in (drops, {}):
            h = dref.encoder(w, toks, mask, ref.TINY, dr)
            assert torch.equal(h, ref.encoder(w, toks, mask, ref.TINY))
            assert torch.equal(dref.pooler(w, h), ref.pooler(w, h))
        wc = ref.make_weights(ref.TINY, 3, prefix="roberta.", pooler=False, num_labels=5, dtype=dt)
        hc = dref.encoder(wc, toks, mask, ref.TINY, {}, prefix="roberta.")
        assert torch.equal(dref.classifier(wc, hc, {}, n), ref.classifier(wc, hc))
        qkv = torch.randn(3, 17, 3 * 64, dtype=dt, generator=torch.Generator().manual_seed(1))
        assert torch.equal(dref.attention(qkv, mask, 2), ref.attention(qkv, mask, 2))


@pytest.mark.parametrize("n_layer", [1, 2, 12])
def test_site_list(n_layer):
    enc, full = dref.site_list(n_layer), dref.site_list(n_layer, head=True)
    assert len(enc) == 3 * n_layer + 1 and len(full) == 3 * n_layer + 3
    assert [s for s, _, _ in full] == list(range(3 * n_layer + 3))  # numbered in the order the forward meets them
    assert [k for _, k, _ in enc].count("attention") == n_layer
    assert all(k == "attention" for s, k, _ in enc if s % 3 == 1) and all(k == "hidden" for s, k, _ in full[-2:])


def test_masks_have_the_sites_shapes_and_rates():
    r, l = 3, 17
    d, nh, n = ref.TINY["d_model"], ref.TINY["n_head"], ref.TINY["n_layer"]
    drops = dref.masks(SEED, 2, ref.TINY, r, l, 0.5, 0.1, head=True)
    assert sorted(drops) == list(range(3 * n + 3))
    assert tuple(drops[0].shape) == (r, l, d) and tuple(drops[1].shape) == (r, nh, l, l)
    assert tuple(drops[3 * n + 1].shape) == (r, d) and tuple(drops[3 * n + 2].shape) == (r, d)
    assert set(drops[0].unique().tolist()) == {0.0, dropout_ref.threshold(0.5)[1]}
    assert abs(float((drops[2] == 0).double().mean()) - 0.5) < 0.05
    assert abs(float((drops[1] == 0).double().mean()) - 0.1) < 0.03
    assert not torch.equal(drops[2], drops[3])  # the site number is part of the counter
    # a dropped probability takes its key out of the sum and nothing else: out = (p o m) v
    qkv = torch.randn(r, l, 3 * d, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    keep = drops[1]
    out = dref.attention(qkv, None, nh, keep)
    assert not torch.equal(out, dref.attention(qkv, None, nh))
    assert torch.equal(dref.attention(qkv, None, nh, torch.ones_like(keep)), dref.attention(qkv, None, nh))


def test_extended_config_defaults_rob_dropout():
    from vidsitu_amd.extended_config import get_cfg

    assert get_cfg({}).mdl.rob_dropout == 0.0
    assert get_cfg({"mdl.rob_dropout": 0.1}).mdl.rob_dropout == 0.1


def test_header_lists_the_new_symbols():
    with open(os.path.join(ROOT, "include", "vidsitu_hip.h")) as f:
        text = f.read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", text), s


def test_signatures_list_the_new_symbols():
    from vidsitu_amd import _lib

    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES, s
    n_fwd, n_drop = len(_lib.SIGNATURES["vs_attn_pad_fwd"][1]), len(_lib.SIGNATURES["vs_attn_pad_drop_fwd"][1])
    assert n_drop == n_fwd + 4  # snap, site, thr, scale in front of the stream
    assert len(_lib.SIGNATURES["vs_attn_pad_drop_bwd"][1]) == len(_lib.SIGNATURES["vs_attn_pad_bwd"][1]) + 4


def test_host_state_of_the_roberta_models(monkeypatch):
    """What needs no GPU: the probabilities are constructor arguments and are refused outside [0, 1); at 0 nothing is
    allocated; the [seed, step] state is the flat-parameter base's (refused inside a capture, no parameter, absent from
    the state dict, set and read back, kept across `.to()`)."""
    from vidsitu_amd import _lib, hf_roberta

    plain = hf_roberta.build("roberta-synth-tiny", hf_roberta.RobertaModelHip)
    zero = hf_roberta.build("roberta-synth-tiny", hf_roberta.RobertaModelHip, hidden_dropout_prob=0.0,
                            attention_probs_dropout_prob=0.0)
    for m in (plain, zero):
        assert m._drop_hid is None and m._drop_att is None and m.dropout_state() is None
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(_lib.VsError):
            hf_roberta.build("roberta-synth-tiny", hf_roberta.RobertaModelHip, hidden_dropout_prob=bad)
        with pytest.raises(_lib.VsError):
            hf_roberta.build("roberta-synth-tiny", hf_roberta.RobertaForSequenceClassificationHip, num_labels=5,
                             attention_probs_dropout_prob=bad)
    m = hf_roberta.build("roberta-synth-tiny", hf_roberta.RobertaForSequenceClassificationHip, num_labels=5,
                         hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.5)
    assert m._drop_hid == dropout_ref.threshold(0.1) and m._drop_att == dropout_ref.threshold(0.5)
    keys = set(m.state_dict())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.VsError, match="the RoBERTa dropout state must exist before a graph capture"):
        m._drop_state_on(torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    torch.manual_seed(123)
    st = m._drop_state_on(torch.device("cpu"))
    torch.manual_seed(123)
    assert st.tolist() == [int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)), 0]
    assert set(m.state_dict()) == keys and not any("drop" in k for k, _ in m.named_buffers())
    assert not any(p is st for p in m.parameters())
    m.set_dropout_state((SEED, 7))
    assert m.dropout_state() == (SEED, 7) and m._drop_state is st  # written in place
    m = m.to(torch.float64)
    assert m._drop_state.dtype == torch.int64 and m.dropout_state() == (SEED, 7)


def test_evrel_models_pass_rob_dropout_on():
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.hf_roberta import _RobertaHip
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    for row in ref.EVREL_NAMES:
        for p in (0.0, 0.1):
            cfg = get_cfg({"task_type": "evrel", "mdl.mdl_name": row, "mdl.rob_mdl_name": "roberta-synth-tiny",
                           "mdl.rob_dropout": p})
            mdl = get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=synth_data.make_comm(cfg))
            rob = [x for x in mdl.modules() if isinstance(x, _RobertaHip)]
            assert len(rob) == 1
            assert (rob[0].hidden_dropout_prob, rob[0].attention_probs_dropout_prob) == (p, p)
            assert (rob[0]._drop_hid is None) == (p == 0.0) and rob[0].dropout_state() is None
