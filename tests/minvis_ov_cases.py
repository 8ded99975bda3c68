"""Test infrastructure: the PRODUCT MinVIS_OV at the sizes of golden g23 (tests/golden/gen_minvis_ov_golden.py: the reference's own
MinVIS_OV on its own CLIP backbone, with the literal toy CLIP of convnext_cases.py behind an `open_clip` stub), the reference's state
dict loaded strictly, for the CPU host-logic test and the GPU parity test."""
import json
import os
import types

import numpy as np
import torch

import convnext_cases as K
from conftest import GOLDEN, Golden

NAME = "toy_test"


def golden():
    g = Golden("g23_minvis_ov")
    return g, g.meta


def state_dict():
    sd = {}
    for part in ("_state_clip", "_state_pd", "_state_dec"):
        z = np.load(os.path.join(GOLDEN, f"g23_minvis_ov{part}.npz"))
        sd.update({k: torch.from_numpy(z[k].copy()) for k in z.files})
    return {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}      # fp16-exact weights, widened


def state_shapes():
    with open(os.path.join(GOLDEN, "ref_state_shapes_minvis_ov.json")) as f:
        return json.load(f)


def metadata(names):
    return types.SimpleNamespace(classes_ov=names, thing_classes_ov=names, thing_dataset_id_to_contiguous_id={i: i for i in range(2)})


def build(ensemble_on_valid_mask, device="cpu", tokenizer=True):
    from dvis_plus_amd import config
    from dvis_plus_amd.convnext import CLIP
    from dvis_plus_amd.meta_architecture import FCCLIPHead, MinVIS_OV
    from dvis_plus_amd.pixel_decoder import MSDeformAttnPixelDecoder
    from dvis_plus_amd.transformer_decoder import VideoMultiScaleMaskedTransformerDecoder_minvis_OV
    g, meta = golden()
    HID = meta["hidden"]
    cfg = config.get_default_cfg()
    backbone = CLIP(cfg, model_cfg=meta["model_cfg"])
    if tokenizer:
        backbone.text_tokenizer = K.toy_tokenizer
    shapes = {k: v for k, v in backbone.output_shape().items() if k.startswith("res")}
    pd = MSDeformAttnPixelDecoder(shapes, transformer_dropout=0.0, transformer_nheads=meta["heads"], transformer_dim_feedforward=meta["ffn"],
                                  transformer_enc_layers=2, conv_dim=HID, mask_dim=HID, norm="GN",
                                  transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    dec = VideoMultiScaleMaskedTransformerDecoder_minvis_OV(
        HID, True, num_classes=5, hidden_dim=HID, num_queries=meta["Q"], nheads=meta["heads"], dim_feedforward=meta["ffn"],
        dec_layers=meta["layers"], pre_norm=False, mask_dim=HID, enforce_input_project=False, clip_embedding_dim=meta["clip_dim"],
        num_frames=2)
    head = FCCLIPHead(shapes, num_classes=5, pixel_decoder=pd, transformer_predictor=dec, transformer_in_feature="multi_scale_pixel_decoder")
    model = MinVIS_OV(backbone=backbone, sem_seg_head=head, criterion=None, num_queries=meta["Q"], object_mask_threshold=0.3,
                      overlap_threshold=0.3, train_metadatas={k: metadata(v) for k, v in meta["train"].items()},
                      test_metadatas={k: metadata(v) for k, v in meta["test"].items()}, size_divisibility=32,
                      pixel_mean=[123.675, 116.280, 103.530], pixel_std=[58.395, 57.120, 57.375], num_frames=2, window_inference=True,
                      geometric_ensemble_alpha=meta["alpha"], geometric_ensemble_beta=meta["beta"],
                      ensemble_on_valid_mask=ensemble_on_valid_mask, test2train={}, task="vis", window_size=meta["window"])
    model.load_state_dict(state_dict(), strict=True)                  # the checkpoint surface: the reference's key names
    return model.eval().to(device), g, meta


def video(g, meta, device="cpu"):
    return {"image": [f.to(device) for f in g.ins["frames"]], "height": meta["out_hw"][0], "width": meta["out_hw"][1], "name": NAME}


def run(model, g, meta, device="cpu"):
    """One eval forward -> (the output dict, the recorded stages)."""
    model.debug_stages = {}
    out = model([video(g, meta, device)])
    return out, model.debug_stages


def check_against_golden(stages, g, tag, tol):
    """Every recorded stage of the reference's forward (tag: "plain" / "valid") against the product's debug stages."""
    want = {k[len(tag) + 1:]: torch.from_numpy(g.z[k].copy()) for k in g.z.files if k.startswith(tag + "/")}
    maps = np.load(os.path.join(GOLDEN, "g23_minvis_ov_maps.npz"))
    cpu = lambda t: t.detach().float().cpu()
    assert list(stages["num_templates"]) == want["num_templates"].tolist()
    torch.testing.assert_close(cpu(stages["text_classifier"]), want["text_classifier"], **tol)
    torch.testing.assert_close(cpu(stages["clip_vis_dense"]), torch.from_numpy(maps["clip_vis_dense"].copy()), **tol)
    torch.testing.assert_close(cpu(stages["pooled_clip_feature"]), want["pooled_clip_feature"], **tol)
    torch.testing.assert_close(cpu(stages["out_vocab_logits"]), want["out_vocab_logits"], **tol)
    torch.testing.assert_close(cpu(stages["pred_logits"]), want["pred_logits"], **tol)             # ensembled, before post_processing
    torch.testing.assert_close(cpu(stages["cls"]), want["post_logits"], **tol)                     # after it
    # the six arguments of inference_video: pred_cls, pred_masks (Q, T, h, w) in aligned order, img_size, height, width, first_resize_size
    torch.testing.assert_close(cpu(stages["cls"]), want["iv_pred_cls"], **tol)
    idx = stages["aligned_indices"]
    ar = torch.arange(idx.shape[0], device=idx.device)[:, None]
    aligned = cpu(stages["pred_masks"][ar, idx].permute(1, 0, 2, 3))
    torch.testing.assert_close(aligned, torch.from_numpy(maps["iv_pred_masks"].copy()), **tol)
    img_size, out_hw, first = stages["sizes"]
    assert [*img_size, *out_hw, *first] == want["iv_sizes"].tolist()
    return want
