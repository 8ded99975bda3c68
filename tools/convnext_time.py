"""Time csrc/dwconv_ln.hip — the first half of a ConvNeXt block — and one CLIP ConvNeXt trunk forward against torch's own op sequence
on the same GPU and the same tensors.

    python tools/convnext_time.py [--calls 20] [--repeats 5] [--out FILE] [--model convnext_large_d_320]

One JSON line per measurement.  A window is --calls back-to-back calls between two hipEvents after 3 warm-up windows, `us` its time
per call; the two paths alternate --repeats times; the line holds the median of the repeats and `spread` = (max - min).
`sequence_over_kernel` > 1: the kernel is faster.
  (a) dwconv7x7_ln   Fn.dwconv7x7_ln_tokens on the token-major map against the reference sequence on the NCHW map: grouped
      F.conv2d (7 x 7, groups = C) + permute + F.layer_norm, at the four stage shapes of a 736 x 1280 frame — (184 x 320, 192),
      (92 x 160, 384), (46 x 80, 768), (23 x 40, 1536) — with B = 1 and 5.  `bound_us`: x + out once over the 8.0 TB/s bench.py uses;
      `share_of_bound` = bound_us / kernel_us.
  (b) trunk   one forward of the package's trunk (convnext.CLIP.extract_features: token-major, fused kernels, NCHW maps out) against
      the literal torch trunk (tests/convnext_cases.py) with the same random weights, B = 1 frame of 736 x 1280.
The literal trunk is the tests' reference model: this tool imports tests/convnext_cases.py (it puts tests/ on sys.path).
`max_abs_diff` compares the two sides' outputs.  No GPU -> the tool fails (it never times a CPU)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from refiner_train_time import alternate                                                    # noqa: E402
from dvis_plus_amd import config, functions as Fn                                           # noqa: E402
from dvis_plus_amd.convnext import CLIP, clip_model_config                                  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 8.0e12
STAGES = ((184, 320, 192), (92, 160, 384), (46, 80, 768), (23, 40, 1536))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--model", default="convnext_large_d_320")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convnext_time.py needs a GPU")
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)
    gen = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        for h, w, C in STAGES:
            conv = nn.Conv2d(C, C, 7, padding=3, groups=C).to(DEV).requires_grad_(False)
            norm = nn.LayerNorm(C, eps=1e-6).to(DEV).requires_grad_(False)
            for B in (1, 5):
                tok = torch.randn(B, h, w, C, generator=gen, device=DEV)
                nchw = tok.permute(0, 3, 1, 2).contiguous()
                kernel = lambda: Fn.dwconv7x7_ln_tokens(tok, conv, norm)
                seq = lambda: F.layer_norm(F.conv2d(nchw, conv.weight, conv.bias, padding=3, groups=C).permute(0, 2, 3, 1), (C,),
                                           norm.weight, norm.bias, norm.eps)
                line = {"step": "dwconv7x7_ln", "B": B, "h": h, "w": w, "C": C, "max_abs_diff": float((kernel() - seq()).abs().max())}
                line.update(alternate((("kernel", kernel), ("sequence", seq)), a.calls, a.repeats))
                line["bound_us"] = round(2 * 4 * B * h * w * C / HBM_BYTES_PER_S * 1e6, 1)
                line["share_of_bound"] = round(line["bound_us"] / line["kernel_us"], 3)
                line["sequence_over_kernel"] = round(line["sequence_us"] / line["kernel_us"], 2)
                emit(line)
                del tok, nchw
                torch.cuda.empty_cache()

        import convnext_cases as K
        mc = clip_model_config(a.model)
        mc = dict(mc, text=(32, 2, 1), context=9, vocab=50)                                    # the text tower is not timed
        lit = K.randomize_(K.LitCLIP(**mc), seed=0).eval().to(DEV)
        cfg = config.get_default_cfg()
        ours = CLIP(cfg, model_cfg=mc)
        ours.clip_model.load_state_dict(lit.state_dict(), strict=True)
        ours = ours.to(DEV)
        frame = torch.randn(1, 3, 736, 1280, generator=gen, device=DEV)
        kernel = lambda: ours.extract_features(frame)["res5"]
        seq = lambda: lit.extract_features(frame)["res5"]
        want = seq()
        line = {"step": "trunk", "model": a.model, "B": 1, "H": 736, "W": 1280, "max_abs_diff": float((kernel() - want).abs().max()),
                "max_abs_res5": float(want.abs().max())}
        line.update(alternate((("kernel", kernel), ("sequence", seq)), max(2, a.calls // 5), a.repeats))
        line["sequence_over_kernel"] = round(line["sequence_us"] / line["kernel_us"], 2)
        emit(line)
        with Fn.x3_disabled():
            line = {"step": "trunk (x3_disabled: exact-fp32 GEMMs)", "model": a.model, "B": 1, "H": 736, "W": 1280,
                    "max_abs_diff": float((kernel() - want).abs().max())}
            line.update(alternate((("kernel", kernel), ("sequence", seq)), max(2, a.calls // 5), a.repeats))
            line["sequence_over_kernel"] = round(line["sequence_us"] / line["kernel_us"], 2)
            emit(line)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
