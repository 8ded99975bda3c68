"""Time the ConvFFN's token-major depthwise convolution under autograd (forward kernel + csrc/dwconv_tokens_backward.hip) against
the reference's composition (adapter.py:61-98), and one full-depth ViT-L backbone training step with either.

    python tools/vit_adapter_train_time.py [--calls 20] [--repeats 5] [--out FILE]

One JSON line per measurement.  A window is --calls back-to-back calls between two hipEvents after 3 warm-up windows, `us` its
time per call; the two paths alternate --repeats times on the same device and the same tensors; the line holds the median of the
repeats and `spread` = (max - min).
Shape: the ViT-L MinVIS stage (configs/dvis_Plus/ytvis19/vit_adapter/MinVIS_VitAdapterL.yaml): IMS_PER_BATCH 8 clips of
SAMPLING_FRAME_NUM 1 frame, crop (384, 600) -> 8 frames of 384 x 608 after padding to the size divisibility of 32; the extractors'
ConvFFN then sees (8, 21 x 12 x 19 = 4 788, 256) tokens in levels 48 x 76, 24 x 38, 12 x 19.
  (a) convffn_dwconv   forward + backward of depthwise 3 x 3 + bias + GELU on that tensor.  kernel: Fn.dwconv3x3_tokens under
      autograd.  composition: three transposed contiguous copies, grouped Conv2d, transposes back, concatenation, GELU, torch autograd.
      `*_peak_bytes`: torch.cuda.max_memory_allocated over ONE forward + backward above what was allocated before it.
      `max_abs_diff` compares the two sides' output and gradients.  Also the backward alone (`backward_only`).
  (b) vitl_backbone_train_step   D2VitAdapterDinoV2("vitl", freeze_backbone=True).train(): forward + a squared loss on res2..res5 +
      backward, `kernel` as shipped, `composition` with DVIS_DWCONV_TOKENS=0, with peak memory over one step.
No GPU -> the tool fails (it never times a CPU)."""
import argparse
import contextlib
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refiner_train_time import alternate                                                    # noqa: E402
from pixel_decoder_train_time import peak_bytes                                             # noqa: E402
from dvis_plus_amd import functions as Fn                                                   # noqa: E402
from dvis_plus_amd.vit_adapter import D2VitAdapterDinoV2                                     # noqa: E402

DEV = "cuda:0"
FRAMES, HP, WP, C = 8, 384, 608, 256


def composition(x, levels, weight, bias):
    B = x.shape[0]
    outs, off = [], 0
    for h, w in levels:
        m = x[:, off:off + h * w].transpose(1, 2).reshape(B, C, h, w).contiguous()
        outs.append(F.conv2d(m, weight, bias, 1, 1, 1, C).flatten(2).transpose(1, 2))
        off += h * w
    return F.gelu(torch.cat(outs, dim=1))


@contextlib.contextmanager
def composition_path():
    prev = os.environ.get("DVIS_DWCONV_TOKENS")
    os.environ["DVIS_DWCONV_TOKENS"] = "0"
    try:
        yield
    finally:
        if prev is None:
            del os.environ["DVIS_DWCONV_TOKENS"]
        else:
            os.environ["DVIS_DWCONV_TOKENS"] = prev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vit_adapter_train_time.py needs a GPU")
    lines = []
    gen = torch.Generator(device=DEV).manual_seed(0)
    H, W = HP // 16, WP // 16
    levels = [(2 * H, 2 * W), (H, W), (H // 2, W // 2)]
    N = sum(h * w for h, w in levels)
    x = torch.randn(FRAMES, N, C, generator=gen, device=DEV).requires_grad_()
    weight = (torch.randn(C, 1, 3, 3, generator=gen, device=DEV) * 0.3).requires_grad_()
    bias = torch.randn(C, generator=gen, device=DEV).requires_grad_()
    go = torch.randn(FRAMES, N, C, generator=gen, device=DEV)
    leaves = [x, weight, bias]

    def kernel():
        return torch.autograd.grad(Fn.dwconv3x3_tokens(x, levels, weight, bias, gelu=True), leaves, go)

    def comp():
        return torch.autograd.grad(composition(x, levels, weight, bias), leaves, go)
    with torch.no_grad():
        err = float((Fn.dwconv3x3_tokens(x, levels, weight, bias, gelu=True) - composition(x, levels, weight, bias)).abs().max())
    err = max([err] + [float((p - q).abs().max()) for p, q in zip(kernel(), comp())])
    line = {"step": "convffn_dwconv", "frames": FRAMES, "tokens": N, "C": C, "levels": levels}
    line.update(alternate((("kernel", kernel), ("composition", comp)), a.calls, a.repeats))
    line["composition_over_kernel"] = round(line["composition_us"] / line["kernel_us"], 2)
    line["kernel_peak_bytes"], line["composition_peak_bytes"] = peak_bytes(kernel), peak_bytes(comp)
    line["max_abs_diff"] = err
    print(json.dumps(line), flush=True)
    lines.append(line)

    out_c = composition(x, levels, weight, bias)
    xd, wd, bd = x.detach(), weight.detach(), bias.detach()
    line = {"step": "convffn_dwconv", "backward_only": True, "frames": FRAMES, "tokens": N, "C": C}
    line.update(alternate((("kernel", lambda: Fn.dwconv3x3_tokens_backward(xd, levels, wd, bd, go, gelu=True)),
                           ("composition", lambda: torch.autograd.grad(out_c, leaves, go, retain_graph=True))), a.calls, a.repeats))
    line["composition_over_kernel"] = round(line["composition_us"] / line["kernel_us"], 2)
    print(json.dumps(line), flush=True)
    lines.append(line)
    del out_c

    torch.manual_seed(0)
    bb = D2VitAdapterDinoV2("vitl", freeze_backbone=True).to(DEV).train()
    with torch.no_grad():
        for n, p in bb.named_parameters():                  # (the offset / weight projections start at zero weights)
            if n.endswith("sampling_offsets.weight"):
                p.normal_(0, 0.02)
            elif n.endswith("attention_weights.weight"):
                p.normal_(0, 0.05)
    images = torch.randn(FRAMES, 3, HP, WP, generator=gen, device=DEV)

    def step():
        bb.zero_grad(set_to_none=True)
        sum(f.square().mean() for f in bb(images).values()).backward()

    def step_composition():
        with composition_path():
            step()
    step()
    grads = {n: p.grad.clone() for n, p in bb.named_parameters() if p.grad is not None}
    step_composition()
    err = max(float((p.grad - grads[n]).abs().max()) for n, p in bb.named_parameters() if p.grad is not None)
    del grads
    line = {"step": "vitl_backbone_train_step", "frames": FRAMES, "size": [HP, WP], "depth": 24, "extractors": 6}
    line.update(alternate((("kernel", step), ("composition", step_composition)), max(1, a.calls // 10), a.repeats))
    line["composition_over_kernel"] = round(line["composition_us"] / line["kernel_us"], 3)
    line["kernel_peak_bytes"], line["composition_peak_bytes"] = peak_bytes(step), peak_bytes(step_composition)
    line["max_abs_grad_diff"] = err
    print(json.dumps(line), flush=True)
    lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
