"""Time the open-vocabulary (FC-CLIP) classification kernels — csrc/mask_pool.hip, csrc/ov_class_logits.hip — against the reference's
own torch op sequence on the same GPU.

    python tools/ov_heads_time.py [--calls 20] [--repeats 5] [--out FILE]

One JSON line per measurement.  A window is --calls back-to-back calls between two hipEvents after 3 warm-up windows, `us` its time
per call; the two paths alternate --repeats times on the same device and the same tensors; the line holds the median of the repeats
and `spread` = (max - min).  `sequence_over_kernel` > 1: the kernel is faster.
  (a) mask_pool   Fn.mask_pool_mean against MaskPooling.forward (ov_dvis/video_mask2former_transformer_decoder_ov.py:45-67: the binary
      float mask, its sum, the division pass and the einsum) at 184 x 320, C = 256, Q = 100 and 200, B = 1 and 5 (the stride-4 map
      of a 720p frame) and at 23 x 40, C = 1536, Q = 100, B = 30 (the CLIP map of a clip).  `bound_us`: x + logits + outputs once
      over 8.0 TB/s; `share_of_bound` = bound_us / kernel_us.
  (b) text_class_logits   Fn.text_class_logits against get_classification_logits (ibid. :17-36: normalize, scale, matmul, one slice +
      max per class, stack) at R = 3000 rows (30 frames x 100 queries), D = 768, N = 2604 templates over 124 + 1 groups.
  (c) ov_ensemble   Fn.ov_ensemble against the op sequence of ov_dvis/meta_architecture_ov.py:605-641 at R = 3000, K = 124, with
      ENSEMBLE_ON_VALID_MASK.  The inputs are at a tenth of CLIP's scale so that the reference's `p ** a` stays finite.
`max_abs_diff` compares the two sides' output.  No GPU -> the tool fails (it never times a CPU)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refiner_train_time import alternate                                                    # noqa: E402
from dvis_plus_amd import functions as Fn                                                   # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 8.0e12


def ref_mask_pooling(x, mask):
    mask = (mask > 0).to(mask.dtype)
    denorm = mask.sum(dim=(-1, -2), keepdim=True) + 1e-8
    return torch.einsum("bchw,bqhw->bqc", x, mask / denorm)


def ref_classification_logits(x, text_classifier, logit_scale, num_templates):
    x = F.normalize(x, dim=-1)
    logit_scale = torch.clamp(logit_scale.exp(), max=100)
    pred_logits = logit_scale * x @ text_classifier.T
    final, cur = [], 0
    for num_t in num_templates[:-1]:
        final.append(pred_logits[:, :, cur: cur + num_t].max(-1).values)
        cur += num_t
    final.append(pred_logits[:, :, -num_templates[-1]:].max(-1).values)
    return torch.stack(final, dim=-1)


def ref_ensemble(mask_cls_results, out_vocab_cls_results, overlapping, alpha, beta, mask_for_pooling_count):
    in_vocab = mask_cls_results[..., :-1].softmax(-1)
    out_probs = out_vocab_cls_results[..., :-1].softmax(-1)
    valid = (mask_for_pooling_count > 0).to(in_vocab.dtype).unsqueeze(-1)
    alpha = torch.ones_like(in_vocab) * alpha * valid
    beta = torch.ones_like(in_vocab) * beta * valid
    seen = (in_vocab ** (1 - alpha) * out_probs ** alpha).log() * overlapping
    unseen = (in_vocab ** (1 - beta) * out_probs ** beta).log() * (1 - overlapping)
    is_void_prob = F.softmax(mask_cls_results, dim=-1)[..., -1:]
    probs = torch.cat([(seen + unseen).softmax(-1) * (1.0 - is_void_prob), is_void_prob], dim=-1)
    return torch.log(probs + 1e-8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ov_heads_time.py needs a GPU")
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)
    gen = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        for B, Q, C, H, W in ((1, 100, 256, 184, 320), (5, 100, 256, 184, 320), (1, 200, 256, 184, 320), (5, 200, 256, 184, 320),
                              (30, 100, 1536, 23, 40)):
            x = torch.randn(B, C, H, W, generator=gen, device=DEV)
            logits = torch.randn(B, Q, H, W, generator=gen, device=DEV)
            kernel = lambda: Fn.mask_pool_mean(x, logits)[0]
            seq = lambda: ref_mask_pooling(x, logits)
            err = float((kernel() - seq()).abs().max())
            plan = Fn.mask_pool_plan(B, Q, C, H, W)
            line = {"step": "mask_pool", "B": B, "Q": Q, "C": C, "H": H, "W": W, "slabs": plan.slabs}
            line.update(alternate((("kernel", kernel), ("sequence", seq)), a.calls, a.repeats))
            nbytes = 4 * (B * C * H * W + B * Q * H * W + B * Q * (C + 1))
            line["bound_us"] = round(nbytes / HBM_BYTES_PER_S * 1e6, 1)
            line["share_of_bound"] = round(line["bound_us"] / line["kernel_us"], 3)
            line["sequence_over_kernel"] = round(line["sequence_us"] / line["kernel_us"], 2)
            line["max_abs_diff"] = err
            emit(line)
            del x, logits
            torch.cuda.empty_cache()

        R, D, K = 3000, 768, 124
        templates = [21] * K + [1]                                                              # 2604 + 1 rows over 124 + 1 groups
        N = sum(templates)
        emb = torch.randn(30, 100, D, generator=gen, device=DEV)
        text = F.normalize(torch.randn(N, D, generator=gen, device=DEV), dim=-1)
        scale = torch.tensor(2.659, device=DEV)
        kernel = lambda: Fn.text_class_logits(emb, text, scale, templates)
        seq = lambda: ref_classification_logits(emb, text, scale, templates)
        line = {"step": "text_class_logits", "R": R, "D": D, "N": N, "groups": len(templates),
                "max_abs_diff": float((kernel() - seq()).abs().max())}
        line.update(alternate((("kernel", kernel), ("sequence", seq)), a.calls, a.repeats))
        line["sequence_over_kernel"] = round(line["sequence_us"] / line["kernel_us"], 2)
        emit(line)

        in_logits = 10 * (2 * torch.rand(30, 100, K + 1, generator=gen, device=DEV) - 1)
        out_logits = 10 * (2 * torch.rand(30, 100, K + 1, generator=gen, device=DEV) - 1)
        overlapping = (torch.rand(K, generator=gen, device=DEV) < 0.5).float()
        count = torch.randint(0, 4, (30, 100), generator=gen, device=DEV, dtype=torch.int32)
        kernel = lambda: Fn.ov_ensemble(in_logits, out_logits, overlapping, 0.4, 0.8, count)
        seq = lambda: ref_ensemble(in_logits, out_logits, overlapping, 0.4, 0.8, count)
        line = {"step": "ov_ensemble", "R": R, "K": K, "max_abs_diff": float((kernel() - seq()).abs().max())}
        line.update(alternate((("kernel", kernel), ("sequence", seq)), a.calls, a.repeats))
        line["sequence_over_kernel"] = round(line["sequence_us"] / line["kernel_us"], 2)
        emit(line)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
