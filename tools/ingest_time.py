"""Time the test-time frame resize (csrc/frame_resize.hip) and the VideoPredictor ingest of a host clip, against the reference's
host recipe.

    python tools/ingest_time.py [--iters 30] [--host-iters 20] [--ref-iters 5] [--kernels-only] [--out FILE]

One JSON line per step:
  kernel   microseconds of one resize_frames_u8 call (median of --iters after 3 warm-up calls, hipEvent timing around the Python
           wrapper) for T = 36 720p -> 480 x 853, T = 36 1080p -> 480 x 853 and T = 30 720p unchanged; clips are rotated so that
           the ones in flight exceed the 256 MiB Infinity Cache.  TB/s over the algorithmic bytes: every input byte read once
           and every output byte written once.
  host     milliseconds of VideoPredictor staging a list of 36 numpy 720p frames into its pinned buffer, the one host-to-device
           copy and the resize, up to a device synchronise (median of --host-iters; the model is a no-op).
  ref      milliseconds of the reference's per-frame recipe on one host thread for the same 36 frames (demo_video/predictor.py:
           239-248: Pillow resize, astype("float32"), transpose; median of --ref-iters).
--kernels-only: only the kernel lines (for a run under rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvis_plus_amd import functions as Fn                    # noqa: E402
from dvis_plus_amd.predictor import VideoPredictor            # noqa: E402

DEV = "cuda:0"
IC_BYTES = 256 << 20


def timed(fn, iters, warmup=3):
    ts = []
    for i in range(iters + warmup):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def kernel_line(T, src, dst, iters):
    per_clip = T * (src[0] * src[1] + dst[0] * dst[1]) * 3
    n = max(2, -(-2 * IC_BYTES // per_clip))                # clips rotated: at least twice the Infinity Cache
    g = torch.Generator(device=DEV).manual_seed(T + src[0])
    clips = [torch.randint(0, 256, (T, *src, 3), generator=g, dtype=torch.uint8, device=DEV) for _ in range(n)]
    outs = [None] * n

    def run(i):
        outs[i % n] = Fn.resize_frames_u8(clips[i % n], dst)
    us = timed(run, iters)
    mb = per_clip / 1e6
    return {"step": "kernel", "T": T, "in": list(src), "out": list(dst), "clips_rotated": n, "us": round(us, 1),
            "MB_read": round(T * src[0] * src[1] * 3 / 1e6, 1), "MB_written": round(T * dst[0] * dst[1] * 3 / 1e6, 1),
            "TB_per_s": round(mb / us, 3)}


class NoModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("pixel_mean", torch.zeros(3, 1, 1, device=DEV))

    def forward(self, batched_inputs):
        return batched_inputs[0]["image"]


def host_lines(host_iters, ref_iters):
    T, (H, W), dst = 36, (720, 1280), (480, 853)
    rng = np.random.default_rng(0)
    clips = [[rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(T)] for _ in range(2)]
    p = VideoPredictor(model=NoModel(), min_size_test=480, max_size_test=1333)
    ts = []
    for i in range(host_iters + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p(clips[i % 2])
        torch.cuda.synchronize()
        if i >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    host_ms = float(np.median(ts))
    ts = []
    for i in range(ref_iters + 1):
        t0 = time.perf_counter()
        for f in clips[i % 2]:
            img = np.asarray(Image.fromarray(f).resize((dst[1], dst[0]), Image.BILINEAR))
            torch.as_tensor(img.astype("float32").transpose(2, 0, 1))
        if i >= 1:
            ts.append((time.perf_counter() - t0) * 1e3)
    ref_ms = float(np.median(ts))
    return [{"step": "host", "T": T, "in": [H, W], "out": list(dst), "ms": round(host_ms, 2),
             "MB_staged": round(T * H * W * 3 / 1e6, 1), "what": "pinned staging + H2D + resize kernel"},
            {"step": "ref", "T": T, "in": [H, W], "out": list(dst), "ms": round(ref_ms, 1),
             "what": "Pillow resize + astype(float32) + transpose per frame, one host thread",
             "ref_over_host": round(ref_ms / host_ms, 1)}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--ref-iters", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ingest_time.py measures on the GPU"
    lines = [kernel_line(36, (720, 1280), (480, 853), a.iters), kernel_line(36, (1080, 1920), (480, 853), a.iters),
             kernel_line(30, (720, 1280), (720, 1280), a.iters)]
    if not a.kernels_only:
        lines += host_lines(a.host_iters, a.ref_iters)
    head = (f"# python tools/ingest_time.py   (kernels: median of {a.iters} calls after 3 warm-up, hipEvent timing around the Python "
            f"wrapper, clips rotated past the Infinity Cache; host: median of {a.host_iters}; ref: median of {a.ref_iters})")
    text = "\n".join([head] + [json.dumps(l) for l in lines]) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
