"""Time the video-metric kernels (csrc/video_metrics.hip) on one 30-frame 720p clip of blocky id maps.

    python tools/metrics_time.py [--iters 50]

Prints one JSON line per kernel: microseconds per clip (median of --iters launches, hipEvent timing) and the effective
bandwidth over the bytes the kernel must read (two int32 maps: 30 x 720 x 1280 x 8 B = 221 MB).  Consecutive launches read
--clips different clips in turn (default 4: 884 MB, past the 256 MiB Infinity Cache), so a launch's maps come from HBM rather
than from the cache the previous launch filled."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvis_plus_amd import functions as Fn    # noqa: E402


def blocky(T, H, W, n, seed, bh, bw):
    g = torch.Generator().manual_seed(seed)
    cells = torch.randint(0, n, (T, H // bh + 2, W // bw + 2), generator=g, dtype=torch.int32)
    cells[1:] = torch.where(torch.rand(cells[1:].shape, generator=g) < 0.8, cells[:1].expand_as(cells[1:]), cells[1:])
    return cells.repeat_interleave(bh, 1).repeat_interleave(bw, 2)[:, :H, :W].contiguous()


def timed(fn, iters, clips):
    for i in range(clips):
        fn(i)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--clips", type=int, default=4)
    args = ap.parse_args()
    T, H, W = 30, 720, 1280
    dev = "cuda:0"
    table = torch.arange(1, 41, dtype=torch.int32, device=dev) * 1000
    gt = [table[blocky(T, H, W, 40, 2 * c, 48, 80).to(dev).long()] for c in range(args.clips)]
    pred = [blocky(T, H, W, 30, 2 * c + 1, 40, 64).to(dev) for c in range(args.clips)]
    sem_g = [(g // 1000) % 124 + 1 for g in gt]
    sem_p = [p % 124 for p in pred]
    nbytes = 2 * T * H * W * 4
    runs = {
        "dvis_pan_pair_hist": lambda i: Fn.pan_pair_hist(gt[i], pred[i], table, 29, check=False),
        "dvis_sem_confusion": lambda i: Fn.sem_confusion(sem_g[i], sem_p[i], 124, check=False),
        "dvis_video_consistency": lambda i: Fn.video_consistency(sem_g[i], sem_p[i], (8, 16)),
    }
    for name, fn in runs.items():
        us = timed(fn, args.iters, args.clips)
        print(json.dumps({"kernel": name, "T": T, "H": H, "W": W, "clips_rotated": args.clips, "us_per_clip": round(us, 1),
                          "GB_per_s": round(nbytes / us / 1e3, 1)}))


if __name__ == "__main__":
    main()
