"""Writes tests/golden/g22_ov_heads{,_mf,_state,_preds,_pooled}.npz and ref_state_shapes_ov_decoder.json from the reference's own
VideoMultiScaleMaskedTransformerDecoder_dvis_OV (ov_dvis/video_mask2former_transformer_decoder_ov.py), imported UNCHANGED, in
eval and in `.train()` under `torch.no_grad()` (how the open-vocabulary tracker / refiner stages run the frozen segmenter).

    python tests/golden/gen_ov_heads_golden.py

Build-machine only; nothing at test time imports this file.  `_ref_import.py` is used as it is; this generator adds its own `ov_dvis`
package stub after `R.install()`.

Setup (the g17 toy on a smaller map): hidden 64, 2 heads, FFN 128, 4 layers, Q = 6, clip_embedding_dim 24; levels 1 x 2, 2 x 4, 4 x 8
and an 8 x 16 mask map — g17's 24 x 48 map and a 16 x 32 one met the fixture condition below at none of 200 and 800 weight seeds
(138 240 and 61 440 logits against 15 360 here), so the map was shrunk —; 4 frames (num_frames 2: `.train()` splits them into 2 clips of 2, eval keeps one clip of 4).  mask_dim is 64 = hidden:
the reference's `_mask_pooling_proj` starts with LayerNorm(hidden_dim) on the pooled MASK features, so the two widths must agree
(they do, 256 = 256, in every open-vocabulary config).  The text classifier has 5 classes with 1 to 3 templates and a 1-row void
group, rows normalised.  Biases, norms and logit_scale are moved off their initial values.  The input maps are rounded to fp16 and
stored as fp16 (exactly: the fp32 tensors the run used are their widening), which keeps every file below the committed-size limit.

Recorded: inputs, state dict (and its shapes as json), every prediction of the `.train()` run (the eval run's outputs too; the
generator asserts that they equal the last prediction), the pooled embeddings and pixel counts of every prediction, a direct
MaskPooling / get_classification_logits run on random inputs, and the geometric ensemble of ov_dvis/meta_architecture_ov.py:603-642,
transcribed below as data flow on recorded inputs (alpha 0.4, beta 0.8, with and without ENSEMBLE_ON_VALID_MASK).

Fixture condition (the generator searches weight seeds from 2200 on): the smallest |stride-4 mask logit| over ALL recorded
predictions is at least 100 x the largest difference of those logits between the fp32 run and an fp64 run of the same module — then
no pixel's mask membership depends on summation order and the recorded counts must be reproduced EXACTLY — and the smallest
|down-sized mask logit| that feeds a layer's attention mask is >= 1e-4 (g17's condition: no attention-mask bit depends on it either).
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_import as R    # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "g22_ov_heads{}.npz")
HID, HEADS, FFN, LAYERS, Q, MD, CLIP = 64, 2, 128, 4, 6, 64, 24
T, VIDEOS, LEVELS, H, W = 2, 2, ((1, 2), (2, 4), (4, 8)), 8, 16
TEMPLATES = (2, 1, 3, 1, 2, 1)            # 5 classes, then the void group
ALPHA, BETA = 0.4, 0.8
MIN_SMALL = 1e-4


def ref_ov():
    R.install()
    if "ov_dvis" not in sys.modules:
        pkg = types.ModuleType("ov_dvis")
        pkg.__path__ = [f"{R.REF}/ov_dvis"]
        sys.modules["ov_dvis"] = pkg
    return R.ref("ov_dvis.video_mask2former_transformer_decoder_ov")


def f16_exact(t):
    return t.half().float()


def inputs():
    gen = torch.Generator().manual_seed(2200)
    N = T * VIDEOS
    x = [f16_exact(torch.randn(N, HID, h, w, generator=gen)) for h, w in LEVELS]
    mask_features = f16_exact(torch.randn(N, MD, H, W, generator=gen))
    text = F.normalize(torch.randn(sum(TEMPLATES), CLIP, generator=gen), dim=-1)
    direct = {"x": torch.randn(2, 8, 5, 7, generator=gen), "mask": torch.randn(2, 3, 5, 7, generator=gen),
              "emb": torch.randn(2, 3, CLIP, generator=gen), "logit_scale": torch.tensor(2.1),
              "clip_pooled": torch.randn(N, Q, CLIP, generator=gen),                 # the CLIP trunk's pooled features stand-in
              "clip_logit_scale": torch.tensor(3.3),
              "overlapping": torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0]),
              "valid": torch.tensor([[3, 0, 7, 1, 0, 2], [0, 5, 5, 0, 9, 1], [1, 1, 0, 4, 2, 0], [6, 0, 0, 2, 3, 8]], dtype=torch.int32)}
    return x, mask_features, text, direct


def ensemble(mask_cls_results, out_vocab_cls_results, overlapping, alpha, beta, valid):
    """ov_dvis/meta_architecture_ov.py:603-642 as data flow (t q c rows; `valid` = the pixel counts of mask_for_pooling or None)."""
    in_vocab_cls_results = mask_cls_results[..., :-1]
    out_vocab_cls_results = out_vocab_cls_results[..., :-1]
    out_vocab_cls_probs = out_vocab_cls_results.softmax(-1)
    in_vocab_cls_results = in_vocab_cls_results.softmax(-1)
    if valid is not None:
        valid_masking = (valid > 0).to(in_vocab_cls_results.dtype).unsqueeze(-1)
        alpha = torch.ones_like(in_vocab_cls_results) * alpha * valid_masking
        beta = torch.ones_like(in_vocab_cls_results) * beta * valid_masking
    seen = (in_vocab_cls_results ** (1 - alpha) * out_vocab_cls_probs ** alpha).log() * overlapping
    unseen = (in_vocab_cls_results ** (1 - beta) * out_vocab_cls_probs ** beta).log() * (1 - overlapping)
    cls_results = seen + unseen
    is_void_prob = F.softmax(mask_cls_results, dim=-1)[..., -1:]
    return torch.log(torch.cat([cls_results.softmax(-1) * (1.0 - is_void_prob), is_void_prob], dim=-1) + 1e-8)


def run(dec, mod, x, mask_features, text, train):
    """One forward under no_grad with spies: (outputs, [(pooled, counts)] per prediction, smallest |down-sized logit| fed to a layer)."""
    pooled, small = [], []

    class Spy(mod.MaskPooling):
        def forward(self, x, mask, return_num=False):
            out = super().forward(x, mask, return_num)
            pooled.append((out.clone(), (mask > 0).sum(dim=(-1, -2)).to(torch.int32)))
            return out

    heads = type(dec).forward_prediction_heads

    def spy_heads(output, mf, attn_mask_target_size, text_classifier, num_templates):
        cls, masks, attn = heads(dec, output, mf, attn_mask_target_size, text_classifier, num_templates)
        small.append(F.interpolate(masks, size=attn_mask_target_size, mode="bilinear", align_corners=False).abs().min().item())
        return cls, masks, attn
    dec.mask_pooling, dec.forward_prediction_heads = Spy(), spy_heads
    dec.train(train)
    with torch.no_grad():
        out = dec([t.to(mask_features.dtype) for t in x], mask_features, None, text_classifier=text.to(mask_features.dtype),
                  num_templates=list(TEMPLATES))
    del dec.forward_prediction_heads
    return out, pooled, min(small[:LAYERS])                             # (the last prediction's mask feeds no layer)


def predictions(out):
    return [(a["pred_logits"], a["pred_masks"]) for a in out["aux_outputs"]] + [(out["pred_logits"], out["pred_masks"])]


def generate(seed):
    mod = ref_ov()
    x, mask_features, text, direct = inputs()
    torch.manual_seed(seed)
    dec = mod.VideoMultiScaleMaskedTransformerDecoder_dvis_OV(
        HID, True, num_classes=len(TEMPLATES) - 1, hidden_dim=HID, num_queries=Q, nheads=HEADS, dim_feedforward=FFN, dec_layers=LAYERS,
        pre_norm=False, mask_dim=MD, enforce_input_project=False, clip_embedding_dim=CLIP, num_frames=T)
    with torch.no_grad():
        for n, p in dec.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape))
        dec.logit_scale.fill_(2.4)
    state = {k: v.clone() for k, v in dec.state_dict().items()}
    out, pooled, small = run(dec, mod, x, mask_features, text, train=True)
    assert len(out["aux_outputs"]) == LAYERS and len(pooled) == LAYERS + 1
    assert small >= MIN_SMALL, f"fixture condition: smallest |down-sized mask logit| {small:.3e} < {MIN_SMALL}"
    out64, _, _ = run(dec.double(), mod, x, mask_features.double(), text, train=True)
    dec.float()
    dec.load_state_dict(state)
    preds = predictions(out)
    smallest = min(m.abs().min().item() for _, m in preds)
    err = max((m.double() - m64).abs().max().item() for (_, m), (_, m64) in zip(preds, predictions(out64)))
    assert smallest >= 100 * err, f"fixture condition: smallest |mask logit| {smallest:.3e} < 100 x fp32-vs-fp64 {err:.3e}"
    ev, ev_pooled, _ = run(dec, mod, x, mask_features, text, train=False)
    N = T * VIDEOS
    # eval is the last prediction of the .train() run in the one-clip layout
    assert torch.equal(ev["pred_logits"][0], out["pred_logits"].flatten(0, 1))
    assert torch.equal(ev["pred_masks"][0].transpose(0, 1), out["pred_masks"].transpose(1, 2).flatten(0, 1))
    assert torch.equal(ev_pooled[-1][0], pooled[-1][0]) and len(ev["aux_outputs"]) == LAYERS

    # direct runs of the two ops, and the ensemble on the eval prediction
    mp = mod.MaskPooling()
    d_pooled, d_denorm = mp(direct["x"], direct["mask"], return_num=True)
    d_logits = mod.get_classification_logits(direct["emb"], text, direct["logit_scale"], list(TEMPLATES))
    in_logits = ev["pred_logits"][0]                                                             # (t, q, K + 1)
    out_logits = mod.get_classification_logits(direct["clip_pooled"], text, direct["clip_logit_scale"], list(TEMPLATES))
    ens = ensemble(in_logits, out_logits, direct["overlapping"], ALPHA, BETA, None)
    ens_valid = ensemble(in_logits, out_logits, direct["overlapping"], ALPHA, BETA, direct["valid"])
    assert torch.isfinite(ens).all() and torch.isfinite(ens_valid).all()

    meta = {"hidden": HID, "heads": HEADS, "ffn": FFN, "layers": LAYERS, "classes": len(TEMPLATES) - 1, "Q": Q, "mask_dim": MD,
            "clip_dim": CLIP, "num_frames": T, "videos": VIDEOS, "levels": LEVELS, "H": H, "W": W, "templates": TEMPLATES,
            "alpha": ALPHA, "beta": BETA, "weight_seed": seed, "smallest_abs_mask_logit": smallest, "fp32_vs_fp64_mask_logit": err,
            "smallest_abs_downsized_logit": small}
    arrays = {f"in/x{i}": t.half().numpy() for i, t in enumerate(x)}
    arrays["in/text"] = text.numpy()
    arrays.update({f"direct/{k}": v.numpy() for k, v in direct.items()})
    arrays.update({"direct/pooled": d_pooled.numpy(), "direct/denorm": d_denorm.numpy(), "direct/logits": d_logits.numpy(),
                   "ens/out_logits": out_logits.numpy(), "ens/plain": ens.numpy(), "ens/valid": ens_valid.numpy()})
    for k in ("pred_logits", "pred_masks", "pred_embds", "pred_embds_without_norm"):
        arrays[f"eval/{k}"] = ev[k].numpy()
    arrays["meta"] = np.array(repr(meta))
    np.savez_compressed(OUT.format(""), **arrays)
    np.savez_compressed(OUT.format("_mf"), mask_features=mask_features.half().numpy())
    np.savez_compressed(OUT.format("_state"), **{k: v.numpy().copy() for k, v in state.items()})
    pred = {}
    for i, (logits, pm) in enumerate(preds):
        pred[f"{i}/pred_logits"], pred[f"{i}/pred_masks"] = logits.numpy(), pm.numpy()
    for k in ("pred_embds", "pred_embds_without_norm"):
        pred[k] = out[k].numpy()
    np.savez_compressed(OUT.format("_preds"), **pred)
    np.savez_compressed(OUT.format("_pooled"), **{f"{i}/pooled": p.numpy() for i, (p, _) in enumerate(pooled)},
                        **{f"{i}/count": c.numpy() for i, (_, c) in enumerate(pooled)})
    with open(os.path.join(HERE, "ref_state_shapes_ov_decoder.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in state.items()}, f, indent=0, sort_keys=True)
    for suffix in ("", "_mf", "_state", "_preds", "_pooled"):
        size = os.path.getsize(OUT.format(suffix))
        assert size < 1 << 20, (suffix, size)
        print("wrote", OUT.format(suffix), size, "bytes")
    print(meta)


def main():
    for seed in range(2200, 2400):
        try:
            return generate(seed)
        except AssertionError as e:
            if "fixture condition" not in str(e):
                raise
            print("seed", seed, ":", e)
    raise SystemExit("no seed met the fixture condition")


if __name__ == "__main__":
    main()
