"""Time the fused MSDeformAttn backward (csrc/msda_backward.hip, msda_fused_bwd_kernel) against the composition it replaces under
autograd, and one pixel-decoder training step with either op in its encoder layers.

    python tools/pixel_decoder_train_time.py [--calls 20] [--repeats 5] [--out FILE]

One JSON line per measurement.  A window is --calls back-to-back calls between two hipEvents after 3 warm-up windows, `us` its
time per call; the two paths alternate --repeats times; the line holds the median of the repeats and `spread` = (max - min).
  (a) msda_fused_backward   the backward alone, both `deterministic` settings, at the 720p frame-layer (S = Lq = 19 320 over 23 x 40,
      46 x 80, 92 x 160; M = 8, D = 32, P = 4) with N = 1 and N = 10 frames, and at the ViT-L extractor shape (46 x 80, M = 16,
      D = 64, L = 1, Lq = 19 320, 4 frames).
      fused: Fn.msda_fused_backward on the raw offset / logit rows.  unfused: torch.autograd.grad through MSDeformAttnFunction, the
      softmax and the location arithmetic — the graph built once outside the window (retain_graph), on the same device tensors.
      `*_peak_bytes`: torch.cuda.max_memory_allocated over ONE forward + backward of either side above what was allocated before it
      (the inputs): what the op keeps for its backward plus the backward's own temporaries and results.
      `max_abs_diff` compares the two sides' gradients.
  (b) pixel_decoder_train_step   forward_features in .train() + a squared loss on mask_features and the three maps + backward:
      conv_dim 256, 6 encoder layers, 8 heads, 10 frames of levels 23 x 40 / 46 x 80 / 92 x 160 plus the stride-4 map (184 x 320);
      `fused` as shipped, `unfused` with MSDeformAttnFunction in the six layers.
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
from dvis_plus_amd import functions as Fn                                                   # noqa: E402
from dvis_plus_amd.pixel_decoder import MSDeformAttnPixelDecoder, r50_input_shape           # noqa: E402

DEV = "cuda:0"
P = 4


@contextlib.contextmanager
def deterministic(flag):
    prev, Fn.MSDA_BWD_DETERMINISTIC = Fn.MSDA_BWD_DETERMINISTIC, "1" if flag else "0"
    try:
        yield
    finally:
        Fn.MSDA_BWD_DETERMINISTIC = prev


@contextlib.contextmanager
def unfused_op():
    """MSDeformAttn.train_forward takes its unfused branch (this tool's baseline only)."""
    ok = Fn.msda_fused_backward_ok
    Fn.msda_fused_backward_ok = lambda *a, **k: False
    try:
        yield
    finally:
        Fn.msda_fused_backward_ok = ok


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixel_decoder_train_time.py needs a GPU")
    lines = []
    gen = torch.Generator(device=DEV).manual_seed(0)
    r50 = [(23, 40), (46, 80), (92, 160)]
    for name, N, shapes, M, D in (("720p frame-layer", 1, r50, 8, 32), ("720p frame-layer", 10, r50, 8, 32),
                                  ("ViT-L extractor", 4, [(46, 80)], 16, 64)):
        L = len(shapes)
        s = torch.as_tensor(shapes, dtype=torch.long, device=DEV)
        lsi = torch.cat((s.new_zeros((1,)), s.prod(1).cumsum(0)[:-1]))
        S, Lq = int(s.prod(1).sum()), 19320
        value = torch.randn(N, S, M, D, generator=gen, device=DEV)
        ref = torch.rand(1, Lq, L, 2, generator=gen, device=DEV)
        off = torch.randn(N * Lq, M * L * P * 2, generator=gen, device=DEV) * 2
        lg = torch.randn(N * Lq, M * L * P, generator=gen, device=DEV)
        go = torch.randn(N, Lq, M * D, generator=gen, device=DEV)
        norm = torch.stack([s[:, 1], s[:, 0]], -1).float()[None, None, None, :, None, :]

        def unfused_forward(v, o, g):
            w = torch.softmax(g.view(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
            loc = ref[:, :, None, :, None, :] + o.view(N, Lq, M, L, P, 2) / norm
            return Fn.MSDeformAttnFunction.apply(v, s, lsi, loc.contiguous(), w.contiguous(), 128)
        for det in (False, True):
            with deterministic(det):
                def fused():
                    return Fn.msda_fused_backward(value, s, lsi, ref, off, lg, go, L, P, deterministic=det)
                leaves = [t.clone().requires_grad_() for t in (value, off, lg)]
                out = unfused_forward(*leaves)

                def unfused():
                    return torch.autograd.grad(out, leaves, go, retain_graph=True)
                err = max(float((x - y).abs().max()) for x, y in zip(fused(), unfused()))
                line = {"step": "msda_fused_backward", "shape": name, "N": N, "S": S, "Lq": Lq, "M": M, "D": D, "L": L, "P": P,
                        "deterministic": det}
                line.update(alternate((("fused", fused), ("unfused", unfused)), a.calls, a.repeats))
                line["unfused_over_fused"] = round(line["unfused_us"] / line["fused_us"], 2)
                del out, leaves

                def whole(op):
                    v, o, g = (t.clone().requires_grad_() for t in (value, off, lg))
                    op(v, o, g).backward(go)
                line["fused_peak_bytes"] = peak_bytes(lambda: whole(lambda v, o, g: Fn.msda_fused(v, s, lsi, ref, o, g, L, P)))
                line["unfused_peak_bytes"] = peak_bytes(lambda: whole(unfused_forward))
                line["max_abs_diff"] = err
            print(json.dumps(line), flush=True)
            lines.append(line)

    B, C = 10, 256
    pd = MSDeformAttnPixelDecoder(r50_input_shape(), transformer_dropout=0.0, transformer_nheads=8, transformer_dim_feedforward=1024,
                                  transformer_enc_layers=6, conv_dim=C, mask_dim=C, norm="GN",
                                  transformer_in_features=["res3", "res4", "res5"], common_stride=4).to(DEV).train()
    with torch.no_grad():
        for layer in pd.transformer.encoder.layers:         # (the offset / weight projections start at zero weights)
            layer.self_attn.sampling_offsets.weight.normal_(0, 0.02)
            layer.self_attn.attention_weights.weight.normal_(0, 0.05)
    feats = {k: torch.randn(B, v.channels, 736 // v.stride, 1280 // v.stride, generator=gen, device=DEV)
             for k, v in r50_input_shape().items()}

    def step():
        pd.zero_grad(set_to_none=True)
        mf, _, ms = pd.forward_features(feats)
        (mf.square().mean() + sum(m.square().mean() for m in ms)).backward()

    def step_unfused():
        with unfused_op():
            step()
    step()
    g_fused = {n: p.grad.clone() for n, p in pd.named_parameters()}
    step_unfused()
    err = max(float((p.grad - g_fused[n]).abs().max()) for n, p in pd.named_parameters())
    line = {"step": "pixel_decoder_train_step", "frames": B, "conv_dim": C, "layers": 6, "levels": r50, "mask_map": [184, 320]}
    line.update(alternate((("fused", step), ("unfused", step_unfused)), max(1, a.calls // 10), a.repeats))
    line["unfused_over_fused"] = round(line["unfused_us"] / line["fused_us"], 2)
    line["fused_peak_bytes"], line["unfused_peak_bytes"] = peak_bytes(step), peak_bytes(step_unfused)
    line["max_abs_grad_diff"] = err
    print(json.dumps(line), flush=True)
    lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
