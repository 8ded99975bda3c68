"""Time the VIS scoring kernels (csrc/vis_metrics.hip) and one whole YTVISEvaluator.process() per video.

    python tools/vis_metrics_time.py [--iters 20] [--cpu-iters 1]

Two shapes: YTVIS (720p, T = 36, P = 10 predicted, G = 6 ground-truth tracks) and OVIS (720p, T = 60, P = 20, G = 20), blocky
masks that move a little from frame to frame.  One JSON line per (shape, step): microseconds (median of --iters, hipEvent timing
around the Python wrapper, host syncs included) and GB/s over the bytes the step must move:
  rle_encode           P T H W bytes read twice (the count pass, then the write pass)
  rle_strings          the run lengths read (4 B each) + the characters written
  rle_decode           G T H W mask bytes written (+ the runs read)
  track_intersections  (P + G) T H W bytes read once
  process              one video through YTVISEvaluator.process() (encode + strings + GT decode + intersections + host copies),
                       against the same call on CPU tensors (the cpu_ops formulations) on this box
Two clips are rotated for the kernels (each larger than the 256 MiB Infinity Cache at these shapes)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvis_plus_amd import cpu_ops                         # noqa: E402
from dvis_plus_amd import functions as Fn                 # noqa: E402
from dvis_plus_amd.evaluation import YTVISEvaluator        # noqa: E402


def tracks(K, T, H, W, seed):
    """(K, T, H, W) bool: each track a union of a few boxes drifting over the frames."""
    g = np.random.default_rng(seed)
    m = np.zeros((K, T, H, W), bool)
    for k in range(K):
        for _ in range(3):
            h, w = int(g.integers(H // 10, H // 3)), int(g.integers(W // 10, W // 3))
            y, x = int(g.integers(0, H - h)), int(g.integers(0, W - w))
            for t in range(T):
                yy, xx = min(H - h, y + t // 3), min(W - w, x + t // 2)
                m[k, t, yy:yy + h, xx:xx + w] = True
    return torch.from_numpy(m)


def timed(fn, iters, clips):
    for i in range(clips):
        fn(i)
    torch.cuda.synchronize()
    times = []
    for i in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i % clips)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2]


def gt_json(gt, H, W, path):
    G, T = gt.shape[:2]
    runs, off, area = cpu_ops.rle_encode(gt.reshape(G * T, H, W))
    chars, soff = cpu_ops.rle_strings(runs, off)
    s = chars.numpy().tobytes()
    anns = [{"id": g + 1, "video_id": 1, "category_id": 1 + g % 3, "iscrowd": 0,
             "segmentations": [{"size": [H, W], "counts": s[soff[g * T + t]:soff[g * T + t + 1]].decode()} for t in range(T)],
             "areas": [int(a) for a in area[g * T:(g + 1) * T]]} for g in range(G)]
    with open(path, "w") as f:
        json.dump({"videos": [{"id": 1, "height": H, "width": W, "length": T}],
                   "categories": [{"id": c, "name": f"c{c}"} for c in (1, 2, 3)], "annotations": anns}, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-iters", type=int, default=1)
    args = ap.parse_args()
    dev = "cuda:0"
    tmp = tempfile.mkdtemp()
    for name, (T, P, G) in (("ytvis", (36, 10, 6)), ("ovis", (60, 20, 20))):
        H, W = 720, 1280
        preds = [tracks(P, T, H, W, 10 * c + 1).to(dev) for c in range(2)]
        gts = [tracks(G, T, H, W, 10 * c + 2) for c in range(2)]
        gts_d = [g.to(dev) for g in gts]
        enc = [Fn.rle_encode(p.reshape(P * T, H, W)) for p in preds]
        genc = [cpu_ops.rle_encode(g.reshape(G * T, H, W)) for g in gts]
        genc = [(r.to(dev), o.to(dev)) for r, o, _ in genc]
        px = T * H * W
        nruns = int(enc[0][0].numel())
        nchars = int(Fn.rle_strings(*enc[0][:2])[0].numel())
        steps = {
            "rle_encode": (lambda i: Fn.rle_encode(preds[i].reshape(P * T, H, W)), 2 * P * px),
            "rle_strings": (lambda i: Fn.rle_strings(enc[i][0], enc[i][1]), 4 * nruns + nchars),
            "rle_decode": (lambda i: Fn.rle_decode(genc[i][0], genc[i][1], H, W), G * px),
            "track_intersections": (lambda i: Fn.track_intersections(preds[i], gts_d[i]), (P + G) * px),
        }
        for step, (fn, nbytes) in steps.items():
            us = timed(fn, args.iters, 2)
            print(json.dumps({"shape": name, "T": T, "H": H, "W": W, "P": P, "G": G, "step": step, "us": round(us, 1),
                              "MB": round(nbytes / 1e6, 1), "GB_per_s": round(nbytes / us / 1e3, 1)}), flush=True)
        path = os.path.join(tmp, f"{name}.json")
        gt_json(gts[0], H, W, path)
        inputs = [{"video_id": 1, "length": T}]
        scores = torch.linspace(0.9, 0.1, P, device=dev)
        labels = torch.arange(P, device=dev) % 3
        ev = YTVISEvaluator("timing", None, False, None, json_file=path, dataset_id_to_contiguous_id={1: 0, 2: 1, 3: 2})
        out = {"pred_scores": scores, "pred_labels": labels, "pred_masks": preds[0]}

        def proc(i):
            ev.reset()
            ev.process(inputs, out)
        us = timed(proc, args.iters, 1)
        ev_cpu = YTVISEvaluator("timing", None, False, None, json_file=path, dataset_id_to_contiguous_id={1: 0, 2: 1, 3: 2},
                                device="cpu")
        out_cpu = {"pred_scores": scores.cpu(), "pred_labels": labels.cpu(), "pred_masks": preds[0].cpu()}
        cpu = []
        for _ in range(args.cpu_iters):
            ev_cpu.reset()
            t0 = time.perf_counter()
            ev_cpu.process(inputs, out_cpu)
            cpu.append((time.perf_counter() - t0) * 1e6)
        ok = (ev_cpu._videos[0][0] == ev._videos[0][0] and np.array_equal(ev_cpu._videos[0][2], ev._videos[0][2]))
        print(json.dumps({"shape": name, "T": T, "H": H, "W": W, "P": P, "G": G, "step": "process", "us": round(us, 1),
                          "cpu_us": round(sorted(cpu)[len(cpu) // 2], 1), "speedup": round(sorted(cpu)[len(cpu) // 2] / us, 1),
                          "cpu_threads": torch.get_num_threads(), "same_tables_as_cpu": bool(ok)}), flush=True)


if __name__ == "__main__":
    main()
