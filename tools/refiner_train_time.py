"""Time the attention backward kernel (csrc/attention_backward.hip) at the temporal refiner's training shapes, and one refiner
training step, each against the same work with the torch composition (cpu_ops.attention under torch autograd, on the GPU) in the
same process.

    python tools/refiner_train_time.py [--calls 50] [--repeats 5] [--out FILE]

One JSON line per measurement.  A window is --calls back-to-back calls between two hipEvents after 3 warm-up windows, `us` its
time per call; the two paths alternate --repeats times; the line holds the median of the repeats and `spread` = (max - min).
  (a) attention_backward   dq, dk, dv of one attention, 8 heads of d = 32:
        over time     Lq = Lk = T in {11, 15, 21}, B = Q in {100, 200}
        over queries  Lq = Lk = Q in {100, 200}, B = T = 21
      hip: Fn.attention_backward(q, k, v, grad_out).  torch: torch.autograd.grad through cpu_ops.attention's graph, built once
      outside the window (retain_graph) — the backward alone, as the kernel is; the probabilities it re-reads were materialised
      by that forward.  `max_abs_diff` compares the two, `bit_identical_calls` two kernel calls.
  (b) refiner_train_step   forward in .train() + a squared loss on every layer's masks and logits + backward: 6 layers, hidden
      256, 8 heads, FFN 2048, T = 21 frames, 100 queries, a 48 x 80 map; `hip` as shipped (forward kernel + backward kernel in the 18
      attentions), `torch` with functions.attention replaced by the torch composition for the step.
No GPU -> the tool fails (it never times a CPU)."""
import argparse
import contextlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvis_plus_amd import cpu_ops                            # noqa: E402
from dvis_plus_amd import functions as Fn                    # noqa: E402
from dvis_plus_amd.refiner import TemporalRefiner            # noqa: E402

DEV = "cuda:0"
HEADS, D = 8, 32
C = HEADS * D


def window_us(fn, calls, warmup=3):
    """Microseconds per call of `calls` back-to-back calls (the last of 1 + warmup windows)."""
    for i in range(warmup + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def alternate(paths, calls, repeats):
    res = {name: [] for name, _ in paths}
    for _ in range(repeats):
        for name, fn in paths:
            res[name].append(window_us(fn, calls))
    line = {}
    for name, _ in paths:
        line[f"{name}_us"] = round(float(np.median(res[name])), 1)
        line[f"{name}_spread_us"] = round(max(res[name]) - min(res[name]), 1)
    return line


@contextlib.contextmanager
def torch_attention():
    """functions.attention = the torch composition, for GPU tensors too (this tool's baseline only)."""
    kernel = Fn.attention
    Fn.attention = lambda q, k, v, nheads, mask=None, allowed_count=None, out=None, short=False: \
        cpu_ops.attention(q, k, v, nheads, mask, allowed_count, out)
    try:
        yield
    finally:
        Fn.attention = kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("refiner_train_time.py needs a GPU")
    lines = []
    gen = torch.Generator(device=DEV).manual_seed(0)
    shapes = [("over_time", T, Q) for T in (11, 15, 21) for Q in (100, 200)] + [("over_queries", Q, 21) for Q in (100, 200)]
    for kind, L, B in shapes:
        q, k, v, go = (torch.randn(L, B, C, generator=gen, device=DEV) for _ in range(4))

        def hip():
            return Fn.attention_backward(q, k, v, go, HEADS)
        leaves = [t.clone().requires_grad_() for t in (q, k, v)]
        out = cpu_ops.attention(*leaves, HEADS)

        def ref():
            return torch.autograd.grad(out, leaves, go, retain_graph=True)
        err = max(float((x - y).abs().max()) for x, y in zip(hip(), ref()))
        same = all(torch.equal(x, y) for x, y in zip(hip(), hip()))
        line = {"step": "attention_backward", "kind": kind, "Lq": L, "Lk": L, "B": B, "heads": HEADS, "d": D}
        line.update(alternate((("hip", hip), ("torch", ref)), a.calls, a.repeats))
        line["torch_over_hip"] = round(line["torch_us"] / line["hip_us"], 2)
        line["GFLOPs"] = round(5 * 2.0 * B * HEADS * L * L * D / line["hip_us"] / 1e3, 1)      # five L x L x d products
        line["max_abs_diff"], line["bit_identical_calls"] = err, same
        print(json.dumps(line), flush=True)
        lines.append(line)
        del out, leaves

    T, Q, LAYERS, H, W = 21, 100, 6, 48, 80
    ref_ = TemporalRefiner(hidden_channel=C, feedforward_channel=2048, num_head=HEADS, decoder_layer_num=LAYERS, mask_dim=C,
                           class_num=40).to(DEV).train()
    ie, fe = (torch.randn(1, C, T, Q, generator=gen, device=DEV) for _ in range(2))
    mf = torch.randn(1, T, C, H, W, generator=gen, device=DEV)

    def step():
        ref_.zero_grad(set_to_none=True)
        out = ref_(ie, fe, mf)
        loss = sum(o["pred_masks"].square().mean() + o["pred_logits"].square().mean() for o in [out] + out["aux_outputs"])
        loss.backward()

    def step_torch():
        with torch_attention():
            step()
    step()
    g_hip = {n: p.grad.clone() for n, p in ref_.named_parameters()}
    step_torch()
    err = max(float((p.grad - g_hip[n]).abs().max()) for n, p in ref_.named_parameters())
    line = {"step": "refiner_train_step", "frames": T, "queries": Q, "layers": LAYERS, "hidden": C, "HW": H * W}
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
