"""Writes tests/golden/g17_decoder_train.npz (+ g17_decoder_train_{state,preds,grads,grads_in}.npz: the split keeps every file below
the size limit) from the reference's own VideoMultiScaleMaskedTransformerDecoder_dvisPlus in TRAINING mode
(dvis_Plus/video_mask2former_transformer_decoder.py:258-379).

    python tests/golden/gen_decoder_train_golden.py

Build-machine only; nothing at test time imports this file.  The reference file is imported UNCHANGED through _ref_import.py,
whose REF is pointed at the reference tree's DVIS_DAQ directory (it holds mask2former, mask2former_video and dvis_Plus).  That copy
returns pred_embds / pred_embds_without_norm WITHOUT the re-id embedding concatenated (the package's class concatenates it, as its
eval forward does: the tests compare the first C channels) and an `image_feats_info` entry that is DVIS-DAQ's and is not recorded.

Setup: hidden 64, 2 heads (d = 32), FFN 128, 4 layers (level 0 is visited twice), 5 classes, Q = 6, mask dim 16, re-id head of 3
layers; num_frames 2 with 2 videos (4 frames: the (b t) split matters); levels 3 x 6, 6 x 12, 12 x 24 (18, 72 and 288 keys) and a
24 x 48 mask map.

Loss: no matcher (no assignment ties) — every one of the L + 1 predictions of pred_masks and pred_logits, the last pred_embds and
pred_reid_embed, each contracted with a recorded, seeded random cotangent and divided by its number of elements.  The mask
cotangent is ONE (b, q, t, h, w) tensor shared by the L + 1 predictions, each with its own recorded weight (`cot/mask_weights`).

Recorded: inputs, state dict, every prediction, every layer's EFFECTIVE attention mask (rows blocked everywhere reset, :296), the
gradients of every parameter, of the three input maps and of mask_features, and in `meta` the run's smallest |down-sized mask
logit| over the layers that use it.  Fixture condition: the first weight seed from 1700 on at which that smallest value is
>= 1e-4 — two orders above the fp32 error of a 64-term contraction at these magnitudes, so no mask bit depends on summation order.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_import as R    # noqa: E402

R.REF = os.path.join(os.path.dirname(R.REF), "DVIS_DAQ")

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "g17_decoder_train{}.npz")
HID, HEADS, FFN, LAYERS, NCLS, Q, MD, REID = 64, 2, 128, 4, 5, 6, 16, 3
T, VIDEOS, LEVELS, H, W = 2, 2, ((3, 6), (6, 12), (12, 24)), 24, 48
MIN_LOGIT = 1e-4


def inputs():
    gen = torch.Generator().manual_seed(1700)
    N = T * VIDEOS
    x = [torch.randn(N, HID, h, w, generator=gen) for h, w in LEVELS]
    mask_features = torch.randn(N, MD, H, W, generator=gen)
    cot = {"masks": torch.randn(VIDEOS, Q, T, H, W, generator=gen),
           "mask_weights": 0.5 + torch.rand(LAYERS + 1, generator=gen),
           "logits": torch.randn(LAYERS + 1, VIDEOS, T, Q, NCLS + 1, generator=gen),
           "embds": torch.randn(VIDEOS, HID, T, Q, generator=gen),
           "reid": torch.randn(VIDEOS, HID, T, Q, generator=gen)}
    return x, mask_features, cot


def loss_of(preds, embds, reid, cot):
    """preds: L + 1 (pred_logits, pred_masks) pairs, the learnable queries' first."""
    mean = lambda z, c: (z * c).sum() / z.numel()
    total = mean(embds, cot["embds"]) + mean(reid, cot["reid"])
    for i, (logits, masks) in enumerate(preds):
        total = total + mean(logits, cot["logits"][i]) + cot["mask_weights"][i] * mean(masks, cot["masks"])
    return total


def main():
    for seed in range(1700, 1780):
        try:
            return generate(seed)
        except AssertionError as e:
            if "fixture condition" not in str(e):
                raise
            print("seed", seed, ":", e)
    raise SystemExit("no seed met the fixture condition")


def generate(seed):
    mod = R.ref("dvis_Plus.video_mask2former_transformer_decoder")
    x, mask_features, cot = inputs()
    torch.manual_seed(seed)
    dec = mod.VideoMultiScaleMaskedTransformerDecoder_dvisPlus(
        HID, True, num_classes=NCLS, hidden_dim=HID, num_queries=Q, nheads=HEADS, dim_feedforward=FFN, dec_layers=LAYERS,
        pre_norm=False, mask_dim=MD, enforce_input_project=False, num_frames=T, num_reid_head_layers=REID, reid_hidden_dim=HID)
    with torch.no_grad():           # biases and norms away from their 0 / 1 initial values: their gradients then test something
        for n, p in dec.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape))
    dec.train()
    calls = []
    heads = dec.forward_prediction_heads

    def spy(output, mask_features, attn_mask_target_size):
        cls, masks, attn = heads(output, mask_features, attn_mask_target_size)
        small = F.interpolate(masks.detach(), size=attn_mask_target_size, mode="bilinear", align_corners=False)
        calls.append((attn.clone(), small.abs().min().item()))              # (before the reset of :296 edits it in place)
        return cls, masks, attn
    dec.forward_prediction_heads = spy
    leaves = [t.clone().requires_grad_() for t in x]
    mf = mask_features.clone().requires_grad_()
    out = dec(leaves, mf)
    assert len(calls) == LAYERS + 1 and len(out["aux_outputs"]) == LAYERS
    smallest = min(c[1] for c in calls[:LAYERS])                            # the last prediction's mask feeds no layer
    assert smallest >= MIN_LOGIT, f"fixture condition: smallest |down-sized mask logit| {smallest:.3e} < {MIN_LOGIT}"
    N = T * VIDEOS
    masks, blocked_rows = {}, 0
    for i, (attn, _) in enumerate(calls[:LAYERS]):
        a = attn.view(N, HEADS, Q, -1)
        assert (a == a[:, :1]).all()
        a = a[:, 0]
        full = a.all(-1, keepdim=True)
        blocked_rows += int(full.sum())
        masks[f"mask/{i}"] = (a & ~full).numpy()
    preds = [(a["pred_logits"], a["pred_masks"]) for a in out["aux_outputs"]] + [(out["pred_logits"], out["pred_masks"])]
    loss_of(preds, out["pred_embds"], out["pred_reid_embed"], cot).backward()

    meta = {"hidden": HID, "heads": HEADS, "ffn": FFN, "layers": LAYERS, "classes": NCLS, "Q": Q, "mask_dim": MD, "reid_layers": REID,
            "num_frames": T, "videos": VIDEOS, "levels": LEVELS, "H": H, "W": W, "weight_seed": seed,
            "smallest_abs_downsized_logit": smallest, "fully_blocked_rows": blocked_rows,
            "open_fraction": [float(1 - m.mean()) for m in masks.values()]}
    arrays = {f"in/x{i}": t.numpy() for i, t in enumerate(x)}
    arrays["in/mask_features"] = mask_features.numpy()
    arrays.update({f"cot/{k}": v.numpy() for k, v in cot.items()})
    arrays.update(masks)
    arrays["loss"] = loss_of(preds, out["pred_embds"], out["pred_reid_embed"], cot).detach().numpy()
    arrays["meta"] = np.array(repr(meta))
    np.savez_compressed(OUT.format(""), **arrays)
    np.savez_compressed(OUT.format("_state"), **{k: v.numpy().copy() for k, v in dec.state_dict().items()})
    pred = {}
    for i, (logits, pm) in enumerate(preds):
        pred[f"{i}/pred_logits"], pred[f"{i}/pred_masks"] = logits.detach().numpy(), pm.detach().numpy()
    for k in ("pred_embds", "pred_embds_without_norm", "pred_reid_embed"):
        pred[k] = out[k].detach().numpy()
    np.savez_compressed(OUT.format("_preds"), **pred)
    grads = {}
    for n, p in dec.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
        grads[n] = p.grad.numpy().copy()
    np.savez_compressed(OUT.format("_grads"), **grads)
    np.savez_compressed(OUT.format("_grads_in"), **{f"x{i}": t.grad.numpy() for i, t in enumerate(leaves)},
                        mask_features=mf.grad.numpy())
    for suffix in ("", "_state", "_preds", "_grads", "_grads_in"):
        print("wrote", OUT.format(suffix), os.path.getsize(OUT.format(suffix)), "bytes")
    print(meta)


if __name__ == "__main__":
    main()
