"""Time the referring tracker's training step and the mask-logit backward kernel (csrc/mask_gemm_backward.hip) alone against
torch.einsum's autograd on the same device tensors.

    python tools/tracker_train_time.py [--iters 10] [--repeats 3] [--out FILE]

Shape: the reference's training shape — T = 5 frames, 100 queries, 6 layers, hidden 256, the stride-4 map of a 720p crop
(184 x 320).  One JSON line per step: median microseconds of --iters calls (hipEvent timing, 3 warm-up calls), repeated --repeats
times alternating the two paths; `us` = the median of the repeats' medians, `spread` = (max - min) of them.
  kernel   grad_embed + row_sum of g (T, 600, HW) and feat (T, 256, HW): Fn.mask_logits_backward  vs  what autograd
           runs for the embeddings' gradient of the forward einsum, written out: torch.einsum("brp,bcp->brc", g, feat) plus
           g.sum(-1) for the row sums; with the bytes of g
           over the HIP time as GB/s and the products as TFLOP/s;
  step     tracker forward in .train() + a squared-logit loss on every layer's masks and logits + backward (the criterion has
           its own tool, tools/criterion_time.py).
No GPU -> the tool fails (it never times a CPU)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvis_plus_amd import functions as Fn                    # noqa: E402
from dvis_plus_amd.tracker import ReferringTracker_noiser    # noqa: E402

DEV = "cuda:0"
T, Q, L, C, H, W = 5, 100, 6, 256, 184, 320


def timed(fn, iters, warmup=3):
    ts = []
    for i in range(iters + warmup):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tracker_train_time.py needs a GPU")
    lines = []
    gen = torch.Generator(device=DEV).manual_seed(0)
    R = L * Q
    g = torch.randn(T, R, H, W, generator=gen, device=DEV)
    feat = torch.randn(T, C, H, W, generator=gen, device=DEV)

    def hip():
        return Fn.mask_logits_backward(g, feat)

    def ref():
        # the backward alone: autograd of out = einsum(emb, feat) is this einsum (+ the row sums the bias gradient needs)
        return torch.einsum("brp,bcp->brc", g.flatten(2), feat.flatten(2)), g.flatten(2).sum(-1)
    with torch.no_grad():
        err = float((hip()[0] - ref()[0]).abs().max())
        same = bool(torch.equal(hip()[0], hip()[0]))
        res = {"hip": [], "torch": []}
        for _ in range(a.repeats):
            for name, fn in (("hip", hip), ("torch", ref)):
                res[name].append(timed(fn, a.iters))
    line = {"step": "mask_logits_backward", "frames": T, "rows": R, "C": C, "HW": H * W}
    for name in ("hip", "torch"):
        line[f"{name}_us"] = round(float(np.median(res[name])), 1)
        line[f"{name}_spread_us"] = round(max(res[name]) - min(res[name]), 1)
    line["torch_over_hip"] = round(line["torch_us"] / line["hip_us"], 2)
    line["g_read_GBps"] = round(g.numel() * 4 / line["hip_us"] / 1e3, 1)
    line["TFLOPs"] = round(2.0 * T * R * C * H * W / line["hip_us"] / 1e6, 1)
    line["max_abs_diff"], line["bit_identical_calls"] = err, same
    print(json.dumps(line), flush=True)
    lines.append(line)
    del g
    torch.cuda.empty_cache()

    trk = ReferringTracker_noiser(hidden_channel=C, feedforward_channel=2048, num_head=8, decoder_layer_num=L, mask_dim=C,
                                  class_num=40, noise_mode="wa", noise_ratio=0.8).to(DEV).train()
    fe = torch.randn(1, C, T, Q, generator=gen, device=DEV)
    mf = feat.unsqueeze(0)

    def step():
        trk.zero_grad(set_to_none=True)
        out = trk(fe, mf, frame_embeds_no_norm=fe)
        loss = sum(o["pred_masks"].square().mean() + o["pred_logits"].square().mean() for o in [out] + out["aux_outputs"])
        loss.backward()
    ts = [timed(step, a.iters) for _ in range(a.repeats)]
    line = {"step": "tracker_train_step", "frames": T, "queries": Q, "layers": L, "HW": H * W,
            "hip_us": round(float(np.median(ts)), 1), "hip_spread_us": round(max(ts) - min(ts), 1)}
    print(json.dumps(line), flush=True)
    lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
