"""Time the masked long-key attention backward (csrc/masked_attention_backward.hip) at the masked-attention decoder's training
shapes, and one decoder training step, each against the same work with the torch composition (cpu_ops.attention under torch
autograd, on the GPU) in the same process.

    python tools/decoder_train_time.py [--calls 20] [--repeats 5] [--out FILE]

One JSON line per measurement.  A window is --calls back-to-back calls between two hipEvents after 3 warm-up windows, `us` its
time per call; the two paths alternate --repeats times; the line holds the median of the repeats and `spread` = (max - min).
  (a) masked_attention_backward   dq, dk, dv of one cross-attention, B = 10 frames, 8 heads of d = 32, a random mask that leaves
      about a quarter of the keys open: (Lq, Lk) in (100, 360), (100, 1440), (100, 5760), (200, 5760) — 100 / 200 queries over a
      stride-32 / 16 / 8 level of a 480 x 768 frame.
      hip: Fn.masked_attention_backward(q, k, v, grad_out, mask, allowed_count).  torch: torch.autograd.grad through
      cpu_ops.attention's graph, built once outside the window (retain_graph) — the backward alone, as the kernel is; the
      probabilities it re-reads were materialised by that forward.  `max_abs_diff` compares the two, `bit_identical_calls` two
      kernel calls.
  (b) decoder_train_step   forward in .train() + a squared loss on all L + 1 predictions + backward: 9 layers, hidden 256, 8 heads,
      FFN 2048, 100 queries, 10 frames (2 clips of 5), levels 15 x 24, 30 x 48, 60 x 96 and a 120 x 192 mask map; `hip` as shipped,
      `torch` with functions.masked_attention replaced by the torch composition for the step.
No GPU -> the tool fails (it never times a CPU)."""
import argparse
import contextlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refiner_train_time import alternate                                                    # noqa: E402
from dvis_plus_amd import cpu_ops                                                           # noqa: E402
from dvis_plus_amd import functions as Fn                                                   # noqa: E402
from dvis_plus_amd.transformer_decoder import VideoMultiScaleMaskedTransformerDecoder_dvisPlus   # noqa: E402

DEV = "cuda:0"
HEADS, D, B = 8, 32, 10
C = HEADS * D


@contextlib.contextmanager
def torch_masked_attention():
    """functions.masked_attention = the torch composition, for GPU tensors too (this tool's baseline only)."""
    kernel = Fn.masked_attention
    Fn.masked_attention = cpu_ops.attention
    try:
        yield
    finally:
        Fn.masked_attention = kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decoder_train_time.py needs a GPU")
    lines = []
    gen = torch.Generator(device=DEV).manual_seed(0)
    for Lq, Lk in ((100, 360), (100, 1440), (100, 5760), (200, 5760)):
        q, k, v, go = (torch.randn(L, B, C, generator=gen, device=DEV) for L in (Lq, Lk, Lk, Lq))
        mask = (torch.rand(B, Lq, Lk, generator=gen, device=DEV) >= 0.25).to(torch.uint8)
        allowed = (mask == 0).sum(-1).to(torch.int32)

        def hip():
            return Fn.masked_attention_backward(q, k, v, go, HEADS, mask, allowed)
        leaves = [t.clone().requires_grad_() for t in (q, k, v)]
        out = cpu_ops.attention(*leaves, HEADS, mask, allowed)

        def ref():
            return torch.autograd.grad(out, leaves, go, retain_graph=True)
        err = max(float((x - y).abs().max()) for x, y in zip(hip(), ref()))
        same = all(torch.equal(x, y) for x, y in zip(hip(), hip()))
        plan = Fn.masked_attention_backward_plan(Lq, Lk, D)
        line = {"step": "masked_attention_backward", "Lq": Lq, "Lk": Lk, "B": B, "heads": HEADS, "d": D,
                "open_fraction": round(float((mask == 0).float().mean()), 3), "key_tiles": plan.n_key_tiles}
        line.update(alternate((("hip", hip), ("torch", ref)), a.calls, a.repeats))
        line["torch_over_hip"] = round(line["torch_us"] / line["hip_us"], 2)
        line["max_abs_diff"], line["bit_identical_calls"] = err, same
        print(json.dumps(line), flush=True)
        lines.append(line)
        del out, leaves

    Q, LAYERS, T = 100, 9, 5
    dec = VideoMultiScaleMaskedTransformerDecoder_dvisPlus(
        C, True, num_classes=40, hidden_dim=C, num_queries=Q, nheads=HEADS, dim_feedforward=2048, dec_layers=LAYERS, pre_norm=False,
        mask_dim=C, enforce_input_project=False, num_frames=T, num_reid_head_layers=3, reid_hidden_dim=C).to(DEV).train()
    x = [torch.randn(B, C, h, w, generator=gen, device=DEV) for h, w in ((15, 24), (30, 48), (60, 96))]
    mf = torch.randn(B, C, 120, 192, generator=gen, device=DEV)

    def step():
        dec.zero_grad(set_to_none=True)
        out = dec(x, mf)
        loss = sum(o["pred_masks"].square().mean() + o["pred_logits"].square().mean() for o in [out] + out["aux_outputs"])
        loss.backward()

    def step_torch():
        with torch_masked_attention():
            step()
    step()
    g_hip = {n: p.grad.clone() for n, p in dec.named_parameters() if p.grad is not None}
    step_torch()
    err = max(float((p.grad - g_hip[n]).abs().max()) for n, p in dec.named_parameters() if p.grad is not None)
    line = {"step": "decoder_train_step", "frames": B, "queries": Q, "layers": LAYERS, "hidden": C, "keys": [360, 1440, 5760],
            "mask_map": [120, 192]}
    line.update(alternate((("hip", step), ("torch", step_torch)), max(1, a.calls // 10), a.repeats))
    line["torch_over_hip"] = round(line["torch_us"] / line["hip_us"], 2)
    line["max_abs_grad_diff"] = err
    print(json.dumps(line), flush=True)
    lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
