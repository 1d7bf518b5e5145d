"""Plugin surface: `(task_type, mdl.mdl_name)` -> `{mdl, loss, evl}` classes.

Mirrors `vidsitu_code/mdl_selector.py:26-73` for the rows of the hot path; names
outside it raise NotImplementedError exactly like an unknown name does upstream
(:46,71,73).
"""
from .mdl_sf_base import (SFBase, SFBase_TxEnc, LossB, LossLambda, SFPreFeats_TxDec, SFPreFeats_TxEncDec,
                          Simple_GPT2_New, Simple_TxDec, Simple_TxEncDec)
from .mdl_evrel import (Simple_EvRel_Roberta, SFPret_SimpleEvRel, SFPret_OnlyVb_SimpleEvRel,
                        SFPret_OnlyVid_SimpleEvRel, Simple_TxEncEvRel)
from .evl_vsitu import EvalB, EvalB_Acc, EvalB_Gen

# `vidsitu_code/mdl_selector.py:47-69`
_EVREL = {"rob_evrel": Simple_EvRel_Roberta, "txe_evrel": Simple_TxEncEvRel, "sfpret_evrel": SFPret_SimpleEvRel,
          "sfpret_vbonly_evrel": SFPret_OnlyVb_SimpleEvRel, "sfpret_onlyvid_evrel": SFPret_OnlyVid_SimpleEvRel}


def get_mdl_loss_eval(cfg):
    assert cfg.task_type in set(["vb", "vb_arg", "evrel", "evforecast"])
    if cfg.task_type == "vb":
        if cfg.mdl.mdl_name == "sf_base":
            return {"mdl": SFBase, "loss": LossB, "evl": EvalB}
        if cfg.mdl.mdl_name == "sf_base_txenc":  # BASELINE config 3 composition
            return {"mdl": SFBase_TxEnc, "loss": LossB, "evl": EvalB}
        raise NotImplementedError
    elif cfg.task_type == "vb_arg":
        if cfg.mdl.mdl_name == "new_gpt2_only":
            return {"mdl": Simple_GPT2_New, "loss": LossLambda, "evl": EvalB_Gen}
        if cfg.mdl.mdl_name == "tx_only":
            return {"mdl": Simple_TxDec, "loss": LossLambda, "evl": EvalB_Gen}
        if cfg.mdl.mdl_name == "txed_only":
            return {"mdl": Simple_TxEncDec, "loss": LossLambda, "evl": EvalB_Gen}
        if cfg.mdl.mdl_name == "sfpret_txed_vbarg":
            return {"mdl": SFPreFeats_TxDec, "loss": LossLambda, "evl": EvalB_Gen}
        if cfg.mdl.mdl_name == "sfpret_txe_txd_vbarg":
            return {"mdl": SFPreFeats_TxEncDec, "loss": LossLambda, "evl": EvalB_Gen}
        raise NotImplementedError
    elif cfg.task_type == "evrel":
        if cfg.mdl.mdl_name in _EVREL:
            return {"mdl": _EVREL[cfg.mdl.mdl_name], "loss": LossLambda, "evl": EvalB_Acc}
        raise NotImplementedError
    else:
        raise NotImplementedError
