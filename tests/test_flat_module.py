"""`vidsitu_amd.flat_module.FlatParamModule` through its three users, without a GPU: state-dict keys and their
order, the load rules (missing / unexpected / tolerated keys, size mismatch), the life of the derived weight copies
(`_wt_epoch`, empty caches after load / `.to()` / `resize_token_embeddings`), parameter order, `KVCacheState.reorder`."""
import pytest
import torch

from vidsitu_amd._lib import VsError


def _gpt2():
    from vidsitu_amd.hf_gpt2_fseq import GPT2_DIMS, GPT2LMHeadModelHip

    return GPT2LMHeadModelHip(*GPT2_DIMS["gpt2-synth-tiny"])


def _txdec():
    from vidsitu_amd.fseq_txdec import TransformerDecoderHip

    return TransformerDecoderHip(vocab=50, d_model=32, ffn=48, n_head=4, n_layer=2, out_dim=16, pad=49)


def _roberta():
    from vidsitu_amd import hf_roberta

    return hf_roberta.build("roberta-synth-tiny", hf_roberta.RobertaModelHip)


def _roberta_cls():
    from vidsitu_amd import hf_roberta

    return hf_roberta.build("roberta-synth-tiny", hf_roberta.RobertaForSequenceClassificationHip, num_labels=5)


# model -> (constructor, number of state-dict keys, the last keys, tolerated foreign keys, a vector parameter)
MODELS = {
    "gpt2": (_gpt2, 29, ["lm_head.weight"],
             ["lm_head.weight", "transformer.h.0.attn.bias", "transformer.h.1.attn.masked_bias"],
             "transformer.ln_f.bias"),
    "txdec": (_txdec, 57, ["embed_positions._float_tensor", "version"], ["embed_positions._float_tensor", "version"],
              "layers.1.final_layer_norm.bias"),
    "roberta": (_roberta, 39, ["pooler.dense.bias"], ["embeddings.position_ids"], "embeddings.LayerNorm.bias"),
    "roberta_cls": (_roberta_cls, 41, ["classifier.out_proj.bias"], ["roberta.embeddings.position_ids"],
                    "roberta.embeddings.LayerNorm.bias"),
}


@pytest.fixture(params=list(MODELS))
def case(request):
    make, n_keys, last, tolerated, vec = MODELS[request.param]
    torch.manual_seed(0)
    return request.param, make(), n_keys, last, tolerated, vec


def test_state_dict_keys_are_the_names_then_the_extras(case):
    name, m, n_keys, last, _, _ = case
    sd = m.state_dict()
    keys = list(sd)
    assert len(keys) == n_keys and keys[-len(last):] == last
    extras = keys[len(m._names):]
    assert keys[:len(m._names)] == m._names and len(extras) == n_keys - len(m._names)
    for k in m._names:
        assert sd[k].data_ptr() == m.P(k).data_ptr() and not sd[k].requires_grad
    if name == "gpt2":
        assert extras == ["lm_head.weight"]
        assert sd["lm_head.weight"].data_ptr() == m.P("transformer.wte.weight").data_ptr()  # tied
    elif name == "txdec":
        assert extras == last and float(sd["version"]) == 3.0
    else:
        assert extras == []
    assert list(m.state_dict(prefix="dec."))[-1] == "dec." + last[-1]


def test_named_parameters_follow_the_names(case):
    name, m, *_ = case
    assert [n for n, _ in m.named_parameters()] == [k.replace(".", "__") for k in m._names]
    if name == "gpt2":
        m.resize_token_embeddings(101)
        assert [n for n, _ in m.named_parameters()] == [k.replace(".", "__") for k in m._names]
        assert tuple(m.P("transformer.wte.weight").shape) == (101, 64)
        assert m.config.vocab_size == 101


def test_strict_load_of_its_own_state_dict(case):
    _, m, _, _, _, _ = case
    sd = {k: v.clone() + 1.0 for k, v in m.state_dict().items()}
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    for k in m._names:
        assert torch.equal(m.P(k).detach(), sd[k]), k


def test_tolerated_keys_pass_and_a_foreign_key_does_not(case):
    _, m, _, _, tolerated, _ = case
    sd = dict(m.state_dict())
    for k in tolerated:
        sd[k] = torch.zeros(1)
    sd["bogus"] = torch.zeros(1)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert missing == [] and unexpected == ["bogus"]
    with pytest.raises(RuntimeError, match="bogus"):
        m.load_state_dict(sd, strict=True)


def test_a_dropped_key_is_the_one_reported_missing(case):
    _, m, _, _, _, vec = case
    sd = dict(m.state_dict())
    del sd[vec]
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert missing == [vec] and unexpected == []


def test_wrong_shape_is_a_size_mismatch(case):
    """The vector parameter is 64 wide for GPT-2 and RoBERTa, 32 for the decoder (d_model = 32 has no 64-wide one)."""
    name, m, _, _, _, vec = case
    sd = dict(m.state_dict())
    sd[vec] = torch.zeros(3)
    before = m.P(vec).detach().clone()
    width = 32 if name == "txdec" else 64
    with pytest.raises(RuntimeError) as err:
        m.load_state_dict(sd, strict=True)
    assert f"size mismatch for {vec}: (3,) vs ({width},)" in str(err.value)
    assert torch.equal(m.P(vec).detach(), before)


def _seed_caches(m):
    assert m._CACHES
    for c in m._CACHES:
        getattr(m, c)["seeded"] = torch.zeros(1)


def _caches_empty(m):
    return all(len(getattr(m, c)) == 0 for c in m._CACHES)


def test_load_move_and_resize_drop_the_copies_and_bump_the_epoch(case):
    name, m, *_ = case
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for _ in range(2):  # every load
        _seed_caches(m)
        e0 = m._wt_epoch
        m.load_state_dict(sd)
        assert m._wt_epoch == e0 + 1 and _caches_empty(m)
    for dtype in (torch.float64, torch.float32):  # there and back
        _seed_caches(m)
        e0 = m._wt_epoch
        m.to(dtype)
        assert m._wt_epoch == e0 + 1 and _caches_empty(m) and m.P(m._names[0]).dtype == dtype
    if name == "gpt2":
        _seed_caches(m)
        e0 = m._wt_epoch
        m.resize_token_embeddings(97)  # the size it has: nothing changes
        assert m._wt_epoch == e0 and not _caches_empty(m)
        m.resize_token_embeddings(101)
        assert m._wt_epoch == e0 + 1 and _caches_empty(m)


CAPTURE_TEXT = {"gpt2": "GPT-2 weight copies must exist before a graph capture (run one eager step first)",
                "txdec": "decoder weight copies must exist before a graph capture (run one eager step)",
                "roberta": "RoBERTa's fused q/k/v weights must exist before a graph capture (run one eager step first)"}


def test_cached_copy_is_built_once_per_device_and_rebuilt_after_a_drop(case, monkeypatch):
    """`torch.cuda.is_current_stream_capturing` needs a device: it is answered here (no capture, then a capture)."""
    name, m, *_ = case
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    cache, ref, built = getattr(m, m._CACHES[0]), m.P(m._names[0]), []

    def make():
        built.append(1)
        return (ref.detach().clone(),)  # a tuple of copies, as the fused q/k/v caches hold

    a = m._copy(cache, "k", ref, make)
    assert m._copy(cache, "k", ref, make) is a and len(built) == 1
    cache["k"] = (torch.zeros(1, device="meta"),)  # a copy left behind on another device
    assert m._copy(cache, "k", ref, make)[0].device == ref.device and len(built) == 2
    m._drop_copies()
    m._copy(cache, "k", ref, make)
    assert len(built) == 3
    # during a stream capture a present copy is served, a build raises with the model's own text
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert m._copy(cache, "k", ref, make) is cache["k"] and len(built) == 3
    with pytest.raises(VsError) as err:
        m._copy(cache, "other", ref, make)
    assert str(err.value) == CAPTURE_TEXT[name.split("_")[0]] and "other" not in cache and len(built) == 3


def test_train_state_hand_over(case):
    _, m, *_ = case
    assert m.take_train_state() is None
    m._saved = st = ("activations",)
    assert m.take_train_state() is st and m._saved is None
    m.put_train_state(st)
    assert m._saved is st


def test_decoder_position_table_is_the_sinusoid_table_and_survives_a_drop(monkeypatch):
    from vidsitu_amd.fseq_txdec import sinusoid_table

    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    m = _txdec()
    t = m._pos_table(torch.device("cpu"))
    assert torch.equal(t, sinusoid_table(49, m.max_positions, 32, "cpu")) and tuple(t.shape) == (1025, 32)
    m._drop_copies()  # the table derives from no parameter
    assert m._pos_table(torch.device("cpu")) is t


def _state(rows=3, n_layer=2, heads=2, lmax=4, dh=2):
    from vidsitu_amd.hf_gpt2_fseq import KVCacheState

    st = KVCacheState()
    st.k = torch.arange(n_layer * rows * heads * lmax * dh, dtype=torch.float32).view(n_layer, rows, heads, lmax, dh)
    st.v = -st.k
    st.len = 2
    return st


def test_kv_reorder_without_a_cache_is_a_no_op_and_an_ancestry_table_refuses():
    from vidsitu_amd.hf_gpt2_fseq import KVCacheState

    order = torch.tensor([2, 0, 0])
    st = KVCacheState()
    st.reorder(order, 2)
    assert st.k is None and st.v is None and st.k2 is None and st.len == 0
    for model in (_gpt2(), _txdec()):  # the models' `reorder_state` are thin callers
        model.reorder_state(st, order)
        assert st.k is None and st.k2 is None
    st = _state()
    st.anc = torch.zeros(3, 4, dtype=torch.int32)
    k = st.k
    with pytest.raises(VsError, match="ancestry"):
        st.reorder(order, 2)
    with pytest.raises(VsError, match="ancestry"):
        _txdec().reorder_state(st, order)
    assert st.k is k and st.k2 is None


def test_kv_reorder_gathers_and_swaps_the_double_buffer():
    """`ops.kv_gather` hands its operands to a HIP kernel and refuses CPU tensors (there is no CPU path): where it
    does, this case is skipped and the gather itself stays with tests/test_gpu_gpt2.py."""
    st = _state()
    k, v, order = st.k.clone(), st.v.clone(), torch.tensor([2, 0, 0])
    try:
        st.reorder(order, 2)
    except VsError as e:
        pytest.skip(f"ops.kv_gather takes GPU tensors only: {e}")
    assert torch.equal(st.k[:, :, :, :2], k[:, order][:, :, :, :2])
    assert torch.equal(st.v[:, :, :, :2], v[:, order][:, :, :, :2])
    assert st.k2 is not None and st.rows == 3
