"""Golden g22 (tests/golden/gen_ov_heads_golden.py: the reference's open-vocabulary `_dvis_OV` decoder in eval and in .train() under
no_grad, a direct MaskPooling / get_classification_logits run and the geometric ensemble) and the helpers both OV test files share."""
import ast
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DVIS_OV, MINVIS_OV = "VideoMultiScaleMaskedTransformerDecoder_dvis_OV", "VideoMultiScaleMaskedTransformerDecoder_minvis_OV"


class G22:
    def __init__(self):
        load = lambda s: np.load(os.path.join(GOLDEN, f"g22_ov_heads{s}.npz"))
        self.z, self._mf, self._state, self.preds, self.pooled = (load(s) for s in ("", "_mf", "_state", "_preds", "_pooled"))
        self.meta = ast.literal_eval(str(self.z["meta"]))
        self.templates = list(self.meta["templates"])

    def t(self, key, z=None):
        return torch.from_numpy(np.asarray((self.z if z is None else z)[key]))

    def state(self):
        return {k: torch.from_numpy(self._state[k]) for k in self._state.files}

    def inputs(self, device="cpu", dtype=torch.float32):
        """(x: 3 maps, mask_features, text classifier): the maps are stored as the fp16 values the generator's fp32 run used."""
        x = [self.t(f"in/x{i}").to(device, dtype) for i in range(3)]
        return x, self.t("mask_features", self._mf).to(device, dtype), self.t("in/text").to(device, dtype)


_g22 = None


def g22():
    global _g22
    if _g22 is None:
        _g22 = G22()
    return _g22


def build_decoder(g, device="cpu", dtype=torch.float32, cls=DVIS_OV):
    from dvis_plus_amd import transformer_decoder as td
    m = g.meta
    dec = getattr(td, cls)(m["hidden"], True, num_classes=m["classes"], hidden_dim=m["hidden"], num_queries=m["Q"], nheads=m["heads"],
                           dim_feedforward=m["ffn"], dec_layers=m["layers"], pre_norm=False, mask_dim=m["mask_dim"],
                           enforce_input_project=False, clip_embedding_dim=m["clip_dim"], num_frames=m["num_frames"])
    dec.load_state_dict(g.state(), strict=True)
    return dec.to(device, dtype)


def run_decoder(g, dec, train, device="cpu", dtype=torch.float32):
    """One forward under no_grad -> (outputs, [(pooled, count)] of every prediction)."""
    x, mf, text = g.inputs(device, dtype)
    dec.train(train)
    dec.debug_pooled = []
    with torch.no_grad():
        out = dec(x, mf, None, text_classifier=text, num_templates=g.templates)
    pooled, dec.debug_pooled = dec.debug_pooled, None
    return out, pooled


def predictions(out):
    return [(a["pred_logits"], a["pred_masks"]) for a in out["aux_outputs"]] + [(out["pred_logits"], out["pred_masks"])]


def check_train_outputs(g, out, pooled, tol):
    """Every prediction, pooled embedding and class logit of the .train() run within `tol`; pixel counts exactly."""
    preds = predictions(out)
    assert len(preds) == g.meta["layers"] + 1 == len(pooled)
    cpu = lambda z: z.detach().cpu().float()
    for i, (logits, masks) in enumerate(preds):
        torch.testing.assert_close(cpu(masks), g.t(f"{i}/pred_masks", g.preds), **tol)
        assert torch.equal(pooled[i][1].cpu(), g.t(f"{i}/count", g.pooled)), f"prediction {i}: pixel counts differ"
        torch.testing.assert_close(cpu(pooled[i][0]), g.t(f"{i}/pooled", g.pooled), **tol)
        torch.testing.assert_close(cpu(logits), g.t(f"{i}/pred_logits", g.preds), **tol)
    for k in ("pred_embds", "pred_embds_without_norm"):
        torch.testing.assert_close(cpu(out[k]), g.t(k, g.preds), **tol)


def check_eval_outputs(g, out, tol):
    assert out["aux_outputs"] == []
    for k in ("pred_logits", "pred_masks", "pred_embds", "pred_embds_without_norm"):
        torch.testing.assert_close(out[k].detach().cpu().float(), g.t(f"eval/{k}"), **tol)


def reference_ensemble(in_logits, out_logits, overlapping, alpha, beta, valid=None):
    """ov_dvis/meta_architecture_ov.py:603-642 read literally (`p ** a`), for float64 tensors: there the powers of softmaxes of
    logits of magnitude 100 do not underflow (exp(-200) is a normal double), so this is the yardstick at CLIP's scale too."""
    assert in_logits.dtype == torch.float64
    p_in, p_out = in_logits[..., :-1].softmax(-1), out_logits[..., :-1].softmax(-1)
    ov = overlapping.to(torch.float64)
    if valid is not None:
        on = (valid > 0).to(torch.float64).unsqueeze(-1)
        alpha, beta = torch.ones_like(p_in) * alpha * on, torch.ones_like(p_in) * beta * on
    c = (p_in ** (1 - alpha) * p_out ** alpha).log() * ov + (p_in ** (1 - beta) * p_out ** beta).log() * (1 - ov)
    p_void = in_logits.softmax(-1)[..., -1:]
    return torch.log(torch.cat([c.softmax(-1) * (1.0 - p_void), p_void], dim=-1) + 1e-8)


def ov_cfg(decoder=DVIS_OV, **fc_clip):
    """A cfg of the toy width carrying MODEL.FC_CLIP.*, for the registries."""
    from dvis_plus_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cfg.MODEL.SEM_SEG_HEAD.merge({"NAME": "FCCLIPHead", "NUM_CLASSES": 5, "CONVS_DIM": 64, "MASK_DIM": 64, "TRANSFORMER_ENC_LAYERS": 1})
    cfg.MODEL.MASK_FORMER.merge({"TRANSFORMER_DECODER_NAME": decoder, "HIDDEN_DIM": 64, "NHEADS": 2, "DIM_FEEDFORWARD": 128,
                                 "DEC_LAYERS": 5, "NUM_OBJECT_QUERIES": 6})
    cfg.MODEL.FC_CLIP.merge({"EMBED_DIM": 24, **fc_clip})
    cfg.INPUT.SAMPLING_FRAME_NUM = 2
    return cfg
