"""Writes tests/golden/g23_minvis_ov{,_state_clip,_state_pd,_state_dec,_maps}.npz and ref_state_shapes_minvis_ov.json from the reference's
own MinVIS_OV (ov_dvis/meta_architecture_ov.py) on its own CLIP backbone (ov_dvis/backbones/clip.py), both imported UNCHANGED.

    python tests/golden/gen_minvis_ov_golden.py

Build-machine only; nothing at test time imports this file.  `_ref_import.py` is used as it is; this generator adds, in its own code,
  * an `open_clip` stub: `create_model_and_transforms` returns the literal toy CLIP of tests/convnext_cases.py, `get_tokenizer` a
    deterministic toy tokenizer (convnext_cases.toy_tokenizer: a hash of the prompt's words into ids 1 .. vocab - 2, the end-of-text id vocab - 1 after them);
  * the further detectron2 names the two files import (comm, BACKBONE_REGISTRY, Backbone, ImageList.from_tensors, ...), placeholders
    for the training-only criterion / matcher, and the `ov_dvis` package stub.
Setup: the toy CLIP (dims 8 .. 64, embed 24, mlp head), the reference's FCCLIPHead with its MSDeformAttnPixelDecoder (conv 64, mask
64, 2 encoder layers) and `_minvis_OV` decoder at the g22 sizes (hidden = mask_dim = 64, 2 heads, FFN 128, 4 layers, Q = 6); two
training datasets (so `additional_void_embedding` exists), one test dataset of 5 classes with 1 - 3 synonyms of which 2 share a
name with the training classes; a 4-frame clip of 60 x 90 (padded to 64 x 96), window inference with windows of 3, output 45 x 70.
The instance attribute `inference_video` is replaced by a recorder.  Every weight and the frames are fp16-exact and stored as fp16
(the fp32 tensors the run used are their widening), which keeps every file below the committed-size limit.

Recorded, once with ENSEMBLE_ON_VALID_MASK false and once true: the text classifier with void and num_templates,
category_overlapping_mask, clip_vis_dense, the pooled CLIP embeddings, the out-vocabulary logits, the ensembled pred_logits before and
after post_processing, and the six arguments `inference_video` received.

Fixture condition (weight seeds from 2300 on): the smallest |mask logit resized to the CLIP map| is at least 1e-3 (no pooled pixel's
membership depends on rounding), and every frame's embedding-matching cost matrix has a unique optimum by a margin of 1e-3."""
import importlib
import itertools
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import as R    # noqa: E402
import convnext_cases as K    # noqa: E402
from gen_golden import _ImageList    # noqa: E402

OUT = os.path.join(HERE, "g23_minvis_ov{}.npz")
HID, HEADS, FFN, LAYERS, Q, CLIP_DIM = 64, 2, 128, 4, 6, 24
T, H, W, OUT_HW, WINDOW = 4, 60, 90, (45, 70), 3
ALPHA, BETA = 0.4, 0.8
TRAIN = {"toy_train_a": ["cat", "dog, puppy", "tree"], "toy_train_b": ["car, automobile", "road"]}
TEST = {"toy_test": ["dog, hound", "bicycle", "tree, plant, bush", "sky", "boat, ship"]}      # dog and tree overlap the training names
MODEL_CFG = K.toy_model_cfg("mlp")


def ref_modules():
    R.ref_meta()                                                        # detectron2.{data,structures,modeling.backbone}, criterion / matcher stubs
    dm = sys.modules["detectron2.modeling"]

    class _Reg(R._Registry):
        pass
    dm.BACKBONE_REGISTRY, dm.Backbone, dm.ShapeSpec = _Reg("BACKBONE"), nn.Module, R._ShapeSpec
    comm = R._mod("detectron2.utils.comm", get_local_rank=lambda: 0, synchronize=lambda: None)
    sys.modules["detectron2.utils"].comm = comm
    sys.modules["detectron2.structures"].ImageList = _ImageList
    sys.modules["detectron2.layers"].DeformConv = None
    sys.modules["mask2former_video.modeling.criterion"].VideoSetCriterion_ov = object
    R._mod("open_clip", create_model_and_transforms=lambda name, pretrained=None: (K.LitCLIP(**MODEL_CFG), None, None),
           get_tokenizer=lambda name: K.toy_tokenizer)
    for name, path in (("ov_dvis", "ov_dvis"), ("ov_dvis.backbones", "ov_dvis/backbones"),
                       ("mask2former.modeling.meta_arch", "mask2former/modeling/meta_arch")):
        if name not in sys.modules:
            pkg = types.ModuleType(name)
            pkg.__path__ = [f"{R.REF}/{path}"]
            sys.modules[name] = pkg
    clip = importlib.import_module("ov_dvis.backbones.clip")
    meta = importlib.import_module("ov_dvis.meta_architecture_ov")
    head = importlib.import_module("mask2former.modeling.meta_arch.mask_former_head")
    pdm = R.ref("mask2former.modeling.pixel_decoder.msdeformattn")
    dec = R.ref("ov_dvis.video_mask2former_transformer_decoder_ov")
    meta.ImageList = _ImageList
    return clip, meta, head, pdm, dec


def f16_exact_(module):
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(p.half().float())
    return module


def build(seed, ensemble_on_valid_mask, state=None):
    clip, meta, head_mod, pdm, dec_mod = ref_modules()
    ns = types.SimpleNamespace
    cfg = ns(MODEL=ns(FC_CLIP=ns(CLIP_MODEL_NAME="convnext_large_d_320", CLIP_PRETRAINED_WEIGHTS="laion2b_s29b_b131k_ft_soup")))
    torch.manual_seed(seed)
    backbone = clip.CLIP(cfg, None)
    K.randomize_(backbone.clip_model, seed)
    dims = MODEL_CFG["dims"]
    SS = R._ShapeSpec
    inp = {f"res{i + 2}": SS(channels=dims[i], stride=4 * 2 ** i) for i in range(4)}
    pd = pdm.MSDeformAttnPixelDecoder(inp, transformer_dropout=0.0, transformer_nheads=HEADS, transformer_dim_feedforward=FFN,
                                      transformer_enc_layers=2, conv_dim=HID, mask_dim=HID, norm="GN",
                                      transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    dec = dec_mod.VideoMultiScaleMaskedTransformerDecoder_minvis_OV(
        HID, True, num_classes=5, hidden_dim=HID, num_queries=Q, nheads=HEADS, dim_feedforward=FFN, dec_layers=LAYERS, pre_norm=False,
        mask_dim=HID, enforce_input_project=False, clip_embedding_dim=CLIP_DIM, num_frames=2)
    with torch.no_grad():
        for layer in pd.transformer.encoder.layers:
            layer.self_attn.sampling_offsets.weight.normal_(0, 0.3)
            layer.self_attn.attention_weights.weight.normal_(0, 0.5)
        for n, p in dec.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape))
        dec.mask_embed.layers[-1].weight.mul_(30)
        dec.logit_scale.fill_(2.4)
    head = head_mod.FCCLIPHead(inp, num_classes=5, pixel_decoder=pd, loss_weight=1.0, ignore_value=-1, transformer_predictor=dec,
                               transformer_in_feature="multi_scale_pixel_decoder")
    md = lambda names: ns(classes_ov=names, thing_classes_ov=names, thing_dataset_id_to_contiguous_id={i: i for i in range(2)})
    model = meta.MinVIS_OV(backbone=backbone, sem_seg_head=head, criterion=None, num_queries=Q, object_mask_threshold=0.3,
                           overlap_threshold=0.3, train_metadatas={k: md(v) for k, v in TRAIN.items()},
                           test_metadatas={k: md(v) for k, v in TEST.items()}, size_divisibility=32,
                           sem_seg_postprocess_before_inference=True, pixel_mean=[123.675, 116.280, 103.530],
                           pixel_std=[58.395, 57.120, 57.375], num_frames=2, window_inference=True, geometric_ensemble_alpha=ALPHA,
                           geometric_ensemble_beta=BETA, ensemble_on_valid_mask=ensemble_on_valid_mask, test2train={}, task="vis")
    with torch.no_grad():
        model.void_embedding.weight.normal_(0, 1)
        model.additional_void_embedding.weight.normal_(0, 1)
    f16_exact_(model)
    if state is not None:
        model.load_state_dict(state, strict=True)
    return model.eval(), meta


def frames():
    g = torch.Generator().manual_seed(231)
    yy, xx = torch.meshgrid(torch.linspace(0, 6.28, H), torch.linspace(0, 6.28, W), indexing="ij")
    out = []
    for t in range(T):
        pat = 127 + 100 * torch.sin(xx * (1 + t % 2) + 0.3 * t) * torch.cos(yy * 2 + 0.2 * t)
        out.append((torch.randint(0, 256, (3, H, W), generator=g).float() * 0.4 + pat[None] * 0.6).to(torch.uint8))
    return torch.stack(out)


def run(model, meta, fr):
    """One eval forward with spies on the values the forward keeps in locals -> dict of recorded tensors."""
    rec = {}
    vpf = model.backbone.visual_prediction_forward
    gcl, interp = meta.get_classification_logits, meta.F.interpolate
    post, match = model.post_processing, model.match_from_embds

    def spy_vpf(x, masks=None):
        rec["pooled_clip_feature"] = vpf(x, masks)
        return rec["pooled_clip_feature"]

    def spy_gcl(x, text_classifier, logit_scale, num_templates=None):
        rec["text_classifier"], rec["num_templates"] = text_classifier, list(num_templates)
        rec["out_vocab_logits"] = gcl(x, text_classifier, logit_scale, num_templates)
        return rec["out_vocab_logits"]

    def spy_post(outputs):
        rec["pred_logits"], rec["clip_vis_dense"] = outputs["pred_logits"][0].clone(), outputs["clip_vis_dense"]
        rec["pred_masks"] = outputs["pred_masks"][0].clone()
        out = post(outputs)
        rec["post_logits"] = out["pred_logits"][0].clone()
        return out

    def spy_match(tgt, cur):
        c = 1 - F.normalize(cur, dim=1) @ F.normalize(tgt, dim=1).T
        best = sorted(sum(c[p[i], i].item() for i in range(len(p))) for p in itertools.permutations(range(len(c))))
        rec["match_margin"] = min(rec.get("match_margin", 1e9), best[1] - best[0])
        return match(tgt, cur)

    def recorder(*args):
        rec["inference_video"] = args
        return None
    model.backbone.visual_prediction_forward, meta.get_classification_logits = spy_vpf, spy_gcl
    model.post_processing, model.match_from_embds, model.inference_video = spy_post, spy_match, recorder
    try:
        with torch.no_grad():
            model([{"image": [f for f in fr], "height": OUT_HW[0], "width": OUT_HW[1], "name": "toy_test"}])
    finally:
        meta.get_classification_logits = gcl
        model.backbone.visual_prediction_forward, model.post_processing, model.match_from_embds = vpf, post, match
    rec["category_overlapping_mask"] = model.category_overlapping_mask
    clip_hw = rec["clip_vis_dense"].shape[-2:]
    pool = F.interpolate(rec["pred_masks"].transpose(0, 1), size=clip_hw, mode="bilinear", align_corners=False)
    rec["mask_for_pooling_min_abs"] = pool.abs().min().item()
    rec["valid_count"] = (pool > 0).sum(dim=(-1, -2)).to(torch.int32)
    return rec


def generate(seed):
    fr = frames()
    model, meta = build(seed, False)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    recs = {}
    for flag in (False, True):
        m, meta = build(seed, flag, state)
        recs[flag] = run(m, meta, fr)
        r = recs[flag]
        assert r["mask_for_pooling_min_abs"] >= 1e-3, f"fixture condition: |mask logit on the CLIP map| {r['mask_for_pooling_min_abs']:.2e}"
        assert r["match_margin"] >= 1e-3, f"fixture condition: matching margin {r['match_margin']:.2e}"
        assert torch.isfinite(r["pred_logits"]).all() and torch.isfinite(r["post_logits"]).all()
    assert (recs[True]["valid_count"] == 0).any() and not torch.equal(recs[True]["pred_logits"], recs[False]["pred_logits"]), \
        "fixture condition: ENSEMBLE_ON_VALID_MASK must matter (a query without a pixel on the CLIP map)"
    arrays = {"in/frames": fr.numpy()}
    for flag, r in recs.items():
        tag = "valid" if flag else "plain"
        cls, masks, img_size, height, width, first = r["inference_video"]
        for k in ("text_classifier", "category_overlapping_mask", "pooled_clip_feature", "out_vocab_logits", "pred_logits", "post_logits",
                  "valid_count"):
            arrays[f"{tag}/{k}"] = r[k].numpy()
        arrays[f"{tag}/num_templates"] = np.array(r["num_templates"], dtype=np.int64)
        arrays[f"{tag}/iv_pred_cls"] = cls.numpy()
        arrays[f"{tag}/iv_sizes"] = np.array([*img_size, height, width, *first], dtype=np.int64)
        if not flag:
            maps = {"clip_vis_dense": r["clip_vis_dense"].numpy(), "iv_pred_masks": masks.numpy()}
        else:
            assert torch.equal(masks, recs[False]["inference_video"][1]) and torch.equal(r["clip_vis_dense"], recs[False]["clip_vis_dense"])
    meta_d = {"hidden": HID, "heads": HEADS, "ffn": FFN, "layers": LAYERS, "Q": Q, "clip_dim": CLIP_DIM, "T": T, "frame_hw": (H, W),
              "out_hw": OUT_HW, "window": WINDOW, "alpha": ALPHA, "beta": BETA, "train": TRAIN, "test": TEST, "model_cfg": MODEL_CFG,
              "weight_seed": seed, "mask_for_pooling_min_abs": recs[False]["mask_for_pooling_min_abs"],
              "match_margin": recs[False]["match_margin"]}
    arrays["meta"] = np.array(repr(meta_d))
    np.savez_compressed(OUT.format(""), **arrays)
    np.savez_compressed(OUT.format("_maps"), **maps)
    parts = {"_state_clip": "backbone.", "_state_pd": "sem_seg_head.pixel_decoder.", "_state_dec": ""}
    left = dict(state)
    for suffix, prefix in parts.items():
        sel = {k: left.pop(k) for k in list(left) if k.startswith(prefix)}
        assert all(torch.equal(v.half().float(), v) for v in sel.values() if v.is_floating_point())
        np.savez_compressed(OUT.format(suffix), **{k: (v.half().numpy() if v.is_floating_point() else v.numpy()) for k, v in sel.items()})
    with open(os.path.join(HERE, "ref_state_shapes_minvis_ov.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in sorted(state.items())}, f, indent=0)
    for suffix in ("", "_maps", *parts):
        size = os.path.getsize(OUT.format(suffix))
        assert size < 1 << 20, (suffix, size)
        print("wrote", OUT.format(suffix), size, "bytes")
    print(meta_d)


def main():
    for seed in range(2300, 2400):
        try:
            return generate(seed)
        except AssertionError as e:
            if "fixture condition" not in str(e):
                raise
            print("seed", seed, ":", e)
    raise SystemExit("no seed met the fixture condition")


if __name__ == "__main__":
    main()
