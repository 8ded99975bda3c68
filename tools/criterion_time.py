"""Time one matching call and one loss_masks forward + backward of the set criterion: the HIP path (csrc/criterion.hip) against
the reference's torch op sequence on the same device tensors.

    python tools/criterion_time.py [--iters 20] [--repeats 5] [--out FILE]

Shapes: Q = 100 / 200, G = 12, T = 1 / 5 / 21, 184 x 320, K = 12 544 (T * K points for the loss rows' P at T frames flattened is
not modelled: every row samples K points, R = G * T rows).  Per shape and step one JSON line: median microseconds of --iters calls
(hipEvent timing, 3 warm-up calls), repeated --repeats times alternating the two paths; `us` = the median of the repeats' medians,
`spread` = (max - min) of them.  "torch" = the sequence written out below: F.grid_sample x 2 -> binary_cross_entropy_with_logits
x 2 -> einsum x 3 -> sigmoid ... for the matching cost (matcher.py:107-151, up to C on the device); oversampled point_sample,
topk, point_sample x 2, bce + dice and their autograd for the losses (criterion.py:150-200).  The solver and the D2H copy of C are
the same on both sides and left out.  No GPU -> the tool fails (it never times a CPU)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvis_plus_amd import functions as Fn                    # noqa: E402

DEV = "cuda:0"
H, W, K, G = 184, 320, 12544, 12


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


def point_sample(x, coords):
    return F.grid_sample(x, 2.0 * coords[:, :, None, :] - 1.0, align_corners=False)[..., 0]


def torch_match_cost(pred, tgt, coords, logits, ids):
    cost_class = -logits.softmax(-1)[:, ids]
    t = point_sample(tgt.to(pred), coords.repeat(tgt.shape[0], 1, 1)).flatten(1)
    x = point_sample(pred, coords.repeat(pred.shape[0], 1, 1)).flatten(1)
    pos = F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction="none")
    neg = F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")
    cost_mask = (torch.einsum("nc,mc->nm", pos, t) + torch.einsum("nc,mc->nm", neg, 1 - t)) / x.shape[1]
    s = x.sigmoid()
    cost_dice = 1 - (2 * torch.einsum("nc,mc->nm", s, t) + 1) / (s.sum(-1)[:, None] + t.sum(-1)[None, :] + 1)
    return 5.0 * cost_mask + 2.0 * cost_class + 5.0 * cost_dice


def pick_points(sample_fn, src, draws):
    unc = -sample_fn(src, draws[0]).abs()
    idx = torch.topk(unc, k=draws[0].shape[1] // 4, dim=1)[1]            # 0.75 K of 3 K
    return torch.cat([torch.gather(draws[0], 1, idx[:, :, None].expand(-1, -1, 2)), draws[1]], dim=1)


def torch_loss_masks(src, tgt, draws, nm):
    with torch.no_grad():
        coords = pick_points(lambda s, c: point_sample(s[:, None], c)[:, 0], src, draws)
        t = point_sample(tgt.to(src)[:, None], coords)[:, 0]
    x = point_sample(src[:, None], coords)[:, 0]
    loss_mask = F.binary_cross_entropy_with_logits(x, t, reduction="none").mean(1).sum() / nm
    s = x.sigmoid()
    loss_dice = (1 - (2 * (s * t).sum(-1) + 1) / (s.sum(-1) + t.sum(-1) + 1)).sum() / nm
    (5.0 * loss_mask + 5.0 * loss_dice).backward()
    return src.grad


def hip_loss_masks(src, tgt, draws, nm):
    with torch.no_grad():
        coords = pick_points(Fn.point_sample, src, draws)
    loss_mask, loss_dice = Fn.point_mask_losses(src, tgt, coords, nm)
    (5.0 * loss_mask + 5.0 * loss_dice).backward()
    return src.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("criterion_time.py needs a GPU")
    lines = []
    g = torch.Generator(device=DEV).manual_seed(0)
    for T in (1, 5, 21):
        for Q in (100, 200):
            pred = torch.randn(Q, T, H, W, generator=g, device=DEV) * 3
            tgt = torch.rand(G, T, H, W, generator=g, device=DEV) > 0.7
            coords = torch.rand(1, K, 2, generator=g, device=DEV)
            logits, ids = torch.randn(Q, 125, generator=g, device=DEV), torch.randint(0, 124, (G,), generator=g, device=DEV)
            R = G * T
            src = pred[:G].flatten(0, 1).clone().requires_grad_(True)
            trows = tgt.flatten(0, 1)
            draws = (torch.rand(R, 3 * K, 2, generator=g, device=DEV), torch.rand(R, K - int(0.75 * K), 2, generator=g, device=DEV))

            def zero_then(fn):
                def run():
                    src.grad = None
                    fn(src, trows, draws, float(G))
                return run
            with torch.no_grad():
                err_c = float((Fn.match_cost(pred, tgt, coords, logits, ids, 2.0, 5.0, 5.0)
                               - torch_match_cost(pred, tgt, coords, logits, ids)).abs().max())
            src.grad = None
            g_hip = hip_loss_masks(src, trows, draws, float(G)).clone()
            src.grad = None
            err_g = float((g_hip - torch_loss_masks(src, trows, draws, float(G))).abs().max())
            steps = {
                "match_cost": (lambda: Fn.match_cost(pred, tgt, coords, logits, ids, 2.0, 5.0, 5.0),
                               lambda: torch_match_cost(pred, tgt, coords, logits, ids), True),
                "loss_masks_fwd_bwd": (zero_then(hip_loss_masks), zero_then(torch_loss_masks), False),
            }
            for step, (hip, ref, nograd) in steps.items():
                res = {"hip": [], "torch": []}
                for _ in range(a.repeats):
                    for name, fn in (("hip", hip), ("torch", ref)):
                        with torch.set_grad_enabled(not nograd):
                            res[name].append(timed(fn, a.iters))
                line = {"step": step, "Q": Q, "G": G, "T": T, "rows": R if step != "match_cost" else None}
                for name in ("hip", "torch"):
                    line[f"{name}_us"] = round(float(np.median(res[name])), 1)
                    line[f"{name}_spread_us"] = round(max(res[name]) - min(res[name]), 1)
                line["torch_over_hip"] = round(line["torch_us"] / line["hip_us"], 2)
                line["max_abs_diff"] = err_c if step == "match_cost" else err_g
                print(json.dumps(line), flush=True)
                lines.append(line)
            del pred, tgt, src, draws
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
