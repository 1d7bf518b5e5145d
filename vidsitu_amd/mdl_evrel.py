"""Event-relation models (`vidsitu_code/mdl_evrel.py`): the five classes under their reference names, state-dict keys
(`rob_mdl.*`, `vid_feat_encoder.{0,2}.*`, `vis_lang_encoder.{0,2}.*`, `vis_lang_classf.{0,2}.*`), input keys and output
dict (`loss`, `mdl_out` [B, 4, n_ann, 5]).

The text encoder is `hf_roberta` (HIP kernels, one autograd node), the MLPs are `HipMLP` (vs_linear_*), the loss is
vs_softmax_xent; concatenation, expand and index-select are torch plumbing.  Events are paired (Ev1, Ev3), (Ev2, Ev3),
(Ev3, Ev4), (Ev3, Ev5): index lists [0, 1, 2, 2] / [2, 2, 3, 4] (`mdl_evrel.py:110-115`).
"""
import torch
from torch import nn

from . import hf_roberta
from .hf_roberta import RobertaForSequenceClassificationHip, RobertaModelHip
from .mdl_sf_base import HipMLP, get_head_dim, hip_cross_entropy

EV_FIRST, EV_SECOND = (0, 1, 2, 2), (2, 2, 3, 4)


def _flat_tokens(toks, mask):
    b, num_ev, num_seq_eg, seq_len = toks.shape
    return (toks.reshape(b * num_ev * num_seq_eg, seq_len).contiguous(),
            mask.reshape(b * num_ev * num_seq_eg, seq_len).contiguous(), (b, num_ev, num_seq_eg))


def _rob_dropout(cfg):
    """`mdl.rob_dropout`: one number for RoBERTa's hidden and attention dropout (0.1 = what `from_pretrained` gives the
    reference)."""
    p = float(cfg.mdl.get("rob_dropout", 0.0))
    return dict(hidden_dropout_prob=p, attention_probs_dropout_prob=p)


def _rob_matmul(cfg):
    """`mdl.rob_matmul`: 'fp32' | 'bf16', the operand precision of the RoBERTa encoder's dense layers."""
    return dict(matmul=str(cfg.mdl.get("rob_matmul", "fp32")))


class Simple_EvRel_Roberta(nn.Module):
    """`mdl_evrel.py:12-50` (`rob_evrel`): RoBERTa sequence classification (5 labels) over the paired SRL text
    `evrel_seq_out` [B, 4, n_ann, 120]."""

    def __init__(self, cfg, comm):
        super().__init__()
        self.full_cfg = cfg
        self.cfg = cfg.mdl
        self.comm = comm
        self.build_model()

    def build_model(self):
        self.rob_mdl = hf_roberta.build(self.full_cfg.mdl.rob_mdl_name, RobertaForSequenceClassificationHip,
                                        num_labels=5, **_rob_dropout(self.full_cfg), **_rob_matmul(self.full_cfg))

    def forward(self, inp):
        src_toks, src_attn_mask, (B, num_ev, num_seq_eg) = _flat_tokens(inp["evrel_seq_out"],
                                                                        inp["evrel_seq_out_lens"])
        (logits,) = hf_roberta.roberta_apply(self.rob_mdl, src_toks, src_attn_mask)
        loss = hip_cross_entropy(logits.view(-1, logits.size(-1)), inp["evrel_labs"].reshape(-1))
        return {"logits": logits, "loss": loss, "mdl_out": logits.view(B, num_ev, num_seq_eg, -1)}


class SFPret_SimpleEvRel(nn.Module):
    """`mdl_evrel.py:53-130` (`sfpret_evrel`): per event, the pooled RoBERTa output of its SRL text
    (`evrel_seq_out_ones` [B, 5, n_ann, 60]) beside the MLP of its pre-extracted video feature; pairs of events are
    classified into the 5 relations."""

    USE_TEXT, USE_VIDEO = True, True

    def __init__(self, cfg, comm):
        super().__init__()
        self.full_cfg = cfg
        self.cfg = cfg.mdl
        self.comm = comm
        self.build_model()

    def build_model(self):
        self.rob_mdl = hf_roberta.build(self.full_cfg.mdl.rob_mdl_name, RobertaModelHip, add_pooling_layer=True,
                                        **_rob_dropout(self.full_cfg), **_rob_matmul(self.full_cfg))
        head_dim = get_head_dim(self.full_cfg)
        hidden = self.rob_mdl.d_model  # 768 for roberta-base: the reference's 1792 = 1024 + 768
        self.vid_feat_encoder = HipMLP(nn.Linear(head_dim, 1024), nn.ReLU(), nn.Linear(1024, 1024))
        self.vis_lang_encoder = HipMLP(nn.Linear(1024 + hidden, 1024), nn.ReLU(), nn.Linear(1024, 1024))
        self.vis_lang_classf = HipMLP(nn.Linear(2048, 1024), nn.ReLU(), nn.Linear(1024, 5))

    def get_src(self, inp):
        return inp["evrel_seq_out_ones"], inp["evrel_seq_out_ones_lens"]

    def forward(self, inp):
        src_toks1, src_attn1 = self.get_src(inp)
        src_toks, src_attn_mask, (B, num_ev, num_seq_eg) = _flat_tokens(src_toks1, src_attn1)
        assert num_ev == 5
        dev = src_toks.device
        if self.USE_TEXT:
            pooler_out = hf_roberta.roberta_apply(self.rob_mdl, src_toks, src_attn_mask)[1]
            pooler_out_5 = pooler_out.view(B, 5, num_seq_eg, pooler_out.size(-1))
        else:
            pooler_out_5 = torch.zeros((B, 5, num_seq_eg, self.rob_mdl.d_model), dtype=torch.float32, device=dev)
        frm_feats = inp["frm_feats"]
        assert frm_feats.size(1) == 5 and inp["vseg_idx"].size(0) == B
        if self.USE_VIDEO:
            vis_out = self.vid_feat_encoder(frm_feats.float())
            vis_out = vis_out.view(B, 5, 1, -1).expand(B, 5, num_seq_eg, -1)
        else:
            vis_out = torch.zeros((B, 5, num_seq_eg, 1024), dtype=torch.float32, device=dev)
        vis_lang_out = self.vis_lang_encoder(torch.cat([vis_out, pooler_out_5], dim=-1).contiguous())
        first = torch.tensor(EV_FIRST, dtype=torch.long, device=dev)
        second = torch.tensor(EV_SECOND, dtype=torch.long, device=dev)
        vis_lang_out3 = torch.cat([vis_lang_out.index_select(1, first), vis_lang_out.index_select(1, second)], dim=-1)
        logits = self.vis_lang_classf(vis_lang_out3.contiguous()).contiguous()
        loss = hip_cross_entropy(logits.view(-1, logits.size(-1)), inp["evrel_labs"].reshape(-1))
        return {"loss": loss, "mdl_out": logits.view(B, num_ev - 1, num_seq_eg, -1)}


class SFPret_OnlyVb_SimpleEvRel(SFPret_SimpleEvRel):
    """`mdl_evrel.py:133-135` (`sfpret_vbonly_evrel`): the text is the verb alone (`evrel_vbonly_out_ones`, 5 tokens)."""

    def get_src(self, inp):
        return inp["evrel_vbonly_out_ones"], inp["evrel_vbonly_out_ones_lens"]


class SFPret_OnlyVid_SimpleEvRel(SFPret_SimpleEvRel):
    """`mdl_evrel.py:138-188` (`sfpret_onlyvid_evrel`): the reference runs RoBERTa and then replaces its output by
    zeros; here the text encoder is not launched at all.  The result is the same; the `rob_mdl.*` parameters keep
    `grad = None` (as they do in the reference, where nothing connects them to the loss)."""

    USE_TEXT = False


class Simple_TxEncEvRel(SFPret_SimpleEvRel):
    """`mdl_evrel.py:191-240` (`txe_evrel`): the reference runs the video-feature MLP and then replaces its output by
    zeros; here `vid_feat_encoder` is not launched at all.  The result is the same; the `vid_feat_encoder.*`
    parameters keep `grad = None` (as in the reference)."""

    USE_VIDEO = False
