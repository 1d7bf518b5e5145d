"""`mdl.rob_matmul` / `_RobertaHip(..., matmul=)` without a GPU: the config default, the refusal of unknown values, the
key's way from the config into every RoBERTa the event-relation rows build, the new C symbols, and the fp64 restatement
of the mode (tests/roberta_bf16_ref.py), which without rounding is tests/roberta_ref.py."""
import os
import re

import pytest
import torch

import roberta_bf16_ref as bref
import roberta_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROB_ROWS = ("rob_evrel", "sfpret_evrel", "sfpret_vbonly_evrel", "sfpret_onlyvid_evrel")


def test_extended_config_defaults_rob_matmul_to_fp32():
    from vidsitu_amd.extended_config import get_cfg

    cfg = get_cfg({"task_type": "evrel", "mdl.mdl_name": "rob_evrel"})
    assert cfg.mdl.rob_matmul == "fp32"
    assert get_cfg({"task_type": "evrel", "mdl.mdl_name": "rob_evrel", "mdl.rob_matmul": "bf16"}).mdl.rob_matmul == "bf16"
    yml = open(os.path.join(ROOT, "configs", "vsitu_cfg.yml")).read()
    assert re.search(r"^  rob_matmul: 'fp32'\s+# addition", yml, re.M)


@pytest.mark.parametrize("cls_name", ["RobertaModelHip", "RobertaForSequenceClassificationHip"])
def test_a_bad_matmul_value_raises_at_construction(cls_name):
    from vidsitu_amd import hf_roberta

    cls = getattr(hf_roberta, cls_name)
    for bad in ("fp16", "BF16", "", None, True):
        with pytest.raises(ValueError, match="matmul"):
            cls(**ref.TINY, matmul=bad)
        with pytest.raises(ValueError, match="matmul"):
            hf_roberta.build("roberta-synth-tiny", cls, matmul=bad)
    assert cls(**ref.TINY).matmul == "fp32"
    assert cls(**ref.TINY, matmul="fp32").matmul == "fp32"
    m = hf_roberta.build("roberta-synth-tiny", cls, matmul="bf16")
    assert m.matmul == "bf16"
    assert set(m.state_dict()) == set(cls(**ref.TINY).state_dict())  # the mode adds no parameter and no buffer


@pytest.mark.parametrize("value", ["fp32", "bf16", None])
@pytest.mark.parametrize("row", ROB_ROWS)
def test_mdl_evrel_passes_the_key_to_every_roberta_it_builds(row, value, monkeypatch):
    from vidsitu_amd import hf_roberta, synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    over = {"task_type": "evrel", "mdl.mdl_name": row, "mdl.rob_mdl_name": "roberta-synth-tiny"}
    if value is not None:
        over["mdl.rob_matmul"] = value
    cfg = get_cfg(over)
    seen, real = [], hf_roberta.build

    def build(name, cls, state_dict=None, **kw):
        seen.append(kw)
        return real(name, cls, state_dict, **kw)

    monkeypatch.setattr(hf_roberta, "build", build)
    mdl = get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=synth_data.make_comm(cfg))
    want = value or "fp32"
    assert len(seen) == 1 and seen[0]["matmul"] == want
    robs = [m for m in mdl.modules() if isinstance(m, hf_roberta._RobertaHip)]
    assert len(robs) == 1 and robs[0].matmul == want


def test_a_bad_config_value_is_refused_when_the_model_is_built():
    from vidsitu_amd import synth_data
    from vidsitu_amd.extended_config import get_cfg
    from vidsitu_amd.mdl_selector import get_mdl_loss_eval

    cfg = get_cfg({"task_type": "evrel", "mdl.mdl_name": "sfpret_evrel", "mdl.rob_mdl_name": "roberta-synth-tiny",
                   "mdl.rob_matmul": "half"})
    with pytest.raises(ValueError, match="matmul"):
        get_mdl_loss_eval(cfg)["mdl"](cfg=cfg, comm=synth_data.make_comm(cfg))


def test_the_strided_entry_points_are_declared_bound_and_exported():
    from vidsitu_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "vidsitu_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name, n_args in (("vs_gemm_bf16_ws", 14), ("vs_gemm_bf16_ld_ws", 16)):
        decl = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", hdr)
        assert decl, f"{name} is not declared in the header"
        assert len(decl.group(1).split(",")) == n_args
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(_lib.SIGNATURES[name][1]) == n_args
    args = [a.strip().split()[-1].lstrip("*") for a in
            re.search(r"\bint vs_gemm_bf16_ws\s*\(([^)]*)\)", hdr).group(1).split(",")]
    assert args == ["a", "b", "bias", "res", "y", "M", "N", "K", "a_kstrided", "b_kstrided", "act", "workspace",
                    "ws_bytes", "stream"]


def test_strided_entry_refuses_bad_arguments_on_the_host():
    """Checked before any launch, so without a GPU too: no pointer here is ever dereferenced."""
    import ctypes

    from vidsitu_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    assert lib.vs_gemm_bf16_ws(None, p, None, None, p, 8, 8, 8, 0, 1, 0, None, 0, None) < 0
    assert lib.vs_gemm_bf16_ws(p, p, None, None, p, 8, 0, 8, 0, 1, 0, None, 0, None) < 0
    assert lib.vs_gemm_bf16_ws(p, p, None, None, p, 8, 8, 8, 0, 1, 3, None, 0, None) < 0
    assert lib.vs_gemm_bf16_ws(p, p, None, None, p, 8, 8, 8, 2, 0, 0, None, 0, None) < 0
    need = lib.vs_gemm_nt_bf16_workspace_bytes(80, 3072, 768)
    assert need > 0
    assert lib.vs_gemm_bf16_ws(p, p, None, None, p, 80, 3072, 768, 0, 1, 0, p, need - 4, None) < 0
    assert b"workspace" in lib.vs_last_error_string()
    assert lib.vs_gemm_bf16_ld_ws(p, p, None, None, p, 8, 8, 8, 1, 1, 4, 8, 0, None, 0, None) < 0  # lda < M


def _inputs():
    toks, mask = ref.golden_inputs(ref.TINY, 3, 23, 13)
    return toks, mask


def test_restatement_without_rounding_is_roberta_ref():
    toks, mask = _inputs()
    w = ref.make_weights(ref.TINY, 31)
    a = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    b = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    ha, hb = ref.encoder(a, toks, mask, ref.TINY), bref.encoder(b, toks, mask, ref.TINY, rnd=False)
    assert torch.equal(ha, hb)
    g = torch.Generator().manual_seed(3)
    wt = torch.randn(ha.shape, generator=g, dtype=torch.float64)
    (ha * wt).sum().backward()
    (hb * wt).sum().backward()
    for k in a:
        if a[k].grad is None:
            assert b[k].grad is None, k
        else:
            assert torch.equal(a[k].grad, b[k].grad), k


def test_restatement_with_rounding_deviates_far_above_fp32_noise():
    """The end-to-end GPU test needs d_ref well above what an fp32 evaluation of the exact model shows."""
    toks, mask = _inputs()
    w = ref.make_weights(ref.TINY, 31)
    exact = ref.encoder(w, toks, mask, ref.TINY)
    rounded = bref.encoder(w, toks, mask, ref.TINY)
    f32 = ref.encoder({k: v.float() for k, v in w.items()}, toks, mask, ref.TINY).double()
    top = float(exact.abs().max())
    d_ref, e32 = float((rounded - exact).abs().max()) / top, float((f32 - exact).abs().max()) / top
    print(f"PARITY roberta bf16 restatement hidden d_ref={d_ref:.3e} fp32 noise={e32:.3e}")
    assert d_ref > 100 * e32


def test_round_bf16_is_torch_bfloat16():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4096, generator=g)
    assert torch.equal(bref.round_bf16(x), x.bfloat16().float())
