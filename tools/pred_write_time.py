"""Time the prediction-file kernels (csrc/pred_write.hip) and one whole VPSPredictionWriter.process() per VIPSeg clip.

    python tools/pred_write_time.py [--iters 20] [--videos 6] [--out FILE]

One 30-frame 720p clip with ~100 segments (blocky regions, 48-pixel cells, ids drifting over the frames).  One JSON line per step:
  pan_segment_stats  microseconds (median of --iters, hipEvent timing around the Python wrapper) and GB/s over the 110.6 MB
                     int32 map read once
  pan_paint_rgb      the same over the map read + the 82.9 MB RGB map written
  sem_paint          the same over the map read + the 27.6 MB class map written (the VSPW writer's kernel)
  d2h                the painted RGB map and the stats table copied into a pinned buffer (ms, GB/s)
  process            wall ms of one VPSPredictionWriter.process() with the PNG pool left running (median over --videos clips)
                     and with the pool drained after each call, against the same call on CPU tensors (device="cpu")
Two clips are rotated for the kernels (each larger than the 256 MiB Infinity Cache together with its output)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvis_plus_amd import functions as Fn                  # noqa: E402
from dvis_plus_amd.pred_writers import VPSPredictionWriter   # noqa: E402

T, H, W, NSEG = 30, 720, 1280, 100
THINGS = 58


def clip(seed):
    g = torch.Generator().manual_seed(seed)
    cell = 48
    cells = torch.randint(1, NSEG + 1, ((H + cell - 1) // cell + 1, (W + cell - 1) // cell + 1), generator=g,
                          dtype=torch.int32)
    frames = []
    for t in range(T):                                      # the regions drift one pixel per frame
        m = cells.repeat_interleave(cell, 0).repeat_interleave(cell, 1)
        frames.append(m[t // 2:t // 2 + H, t:t + W])
    return torch.stack(frames).contiguous()


def segments(seed):
    g = np.random.default_rng(seed)
    cats = g.integers(0, 124, NSEG)
    return [{"id": i + 1, "isthing": bool(c < THINGS), "category_id": int(c)} for i, c in enumerate(cats)]


def timed(fn, iters):
    ts = []
    for i in range(iters + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        if i >= 2:
            ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--videos", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    clips = [clip(s).to(dev) for s in (1, 2)]
    lut = torch.randint(0, 1 << 24, (NSEG + 1,), dtype=torch.int32).to(dev)
    slut = torch.arange(256, dtype=torch.int32).to(dev)
    map_mb, rgb_mb = T * H * W * 4 / 1e6, T * H * W * 3 / 1e6
    lines = []

    def emit(d):
        d = {"T": T, "H": H, "W": W, "segments": NSEG, **d}
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    us = timed(lambda i: Fn.pan_segment_stats(clips[i % 2], NSEG), args.iters)
    emit({"step": "pan_segment_stats", "us": round(us, 1), "MB": round(map_mb, 1), "GB_per_s": round(map_mb / us * 1e3, 1)})
    us = timed(lambda i: Fn.pan_paint_rgb(clips[i % 2], lut), args.iters)
    emit({"step": "pan_paint_rgb", "us": round(us, 1), "MB": round(map_mb + rgb_mb, 1),
          "GB_per_s": round((map_mb + rgb_mb) / us * 1e3, 1)})
    us = timed(lambda i: Fn.sem_paint(clips[i % 2], slut), args.iters)
    emit({"step": "sem_paint", "us": round(us, 1), "MB": round(map_mb + rgb_mb / 3, 1),
          "GB_per_s": round((map_mb + rgb_mb / 3) / us * 1e3, 1)})

    rgb = Fn.pan_paint_rgb(clips[0], lut)
    stats, _ = Fn.pan_segment_stats(clips[0], NSEG)
    host = torch.empty(rgb.numel() + stats.numel() * 8, dtype=torch.uint8, pin_memory=True)

    def copy(_):
        host[:rgb.numel()].view(rgb.shape).copy_(rgb, non_blocking=True)
        host[rgb.numel():].view(torch.int64).view(stats.shape).copy_(stats, non_blocking=True)
    us = timed(copy, args.iters)
    nbytes = rgb.numel() + stats.numel() * 8
    emit({"step": "d2h", "ms": round(us / 1e3, 3), "MB": round(nbytes / 1e6, 1), "GB_per_s": round(nbytes / 1e3 / us, 1)})

    cats = {i: {"id": i, "isthing": int(i < THINGS), "color": [i, 100, 200]} for i in range(124)}
    kw = dict(categories=cats, thing_dataset_id_to_contiguous_id={i: i for i in range(THINGS)},
              stuff_dataset_id_to_contiguous_id={i: i for i in range(THINGS, 124)})
    segs = segments(3)
    names = [f"{t:05d}.jpg" for t in range(T)]

    def run(writer, pan, k, drain):
        np.random.seed(k)
        t0 = time.perf_counter()
        writer.process([{"video_id": f"v{k}", "file_names": names, "frame_idx": list(range(T))}],
                       {"image_size": (H, W), "pred_masks": pan, "segments_infos": segs})
        if drain:
            writer._png.drain()
        return (time.perf_counter() - t0) * 1e3

    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for drain in (False, True):
            w = VPSPredictionWriter("timing", None, False, os.path.join(tmp, f"d{int(drain)}"), device=dev, **kw)
            w.reset()
            run(w, clips[0], 0, True)                       # warm-up: pool threads, pinned buffer
            res[drain] = float(np.median([run(w, clips[k % 2], k + 1, drain) for k in range(args.videos)]))
            w.evaluate()
        w = VPSPredictionWriter("timing", None, False, os.path.join(tmp, "cpu"), device="cpu", **kw)
        w.reset()
        cpu_pan = clips[0].cpu()
        cpu_ms = run(w, cpu_pan, 0, True)
        w.evaluate()
        same = all(open(os.path.join(tmp, "cpu", "pan_pred", "v0", n), "rb").read() ==
                   open(os.path.join(tmp, "d1", "pan_pred", "v0", n), "rb").read() for n in os.listdir(
                       os.path.join(tmp, "cpu", "pan_pred", "v0")))
    emit({"step": "process", "ms_pool_running": round(res[False], 2), "ms_pool_drained": round(res[True], 2),
          "cpu_ms_pool_drained": round(cpu_ms, 1), "encode_threads": w._png.threads, "same_files_as_cpu": same})
    if args.out:
        with open(args.out, "w") as f:
            f.write("# python tools/pred_write_time.py   (kernels: median of %d calls, hipEvent timing around the Python wrappers; "
                    "two clips rotated; process: median of %d clips)\n" % (args.iters, args.videos))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
