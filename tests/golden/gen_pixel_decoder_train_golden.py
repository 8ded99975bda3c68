"""Writes tests/golden/g18_pixel_decoder_train.npz (+ g18_pixel_decoder_train_{state,grads}.npz: the split keeps every file below
the size limit) from the reference's own MSDeformAttnPixelDecoder in TRAINING mode
(mask2former/modeling/pixel_decoder/msdeformattn.py:314-358), imported UNCHANGED through _ref_import.py.  On the CPU the reference
reaches its torch formulation of the sampling op (ops/modules/ms_deform_attn.py:116-121), as g2 / g7 rely on.

    python tests/golden/gen_pixel_decoder_train_golden.py

Build-machine only; nothing at test time imports this file.

Setup: toy channels 8 / 12 / 16 / 20 at strides 4 / 8 / 16 / 32, conv_dim 64, 2 heads (d = 32), FFN 128, 2 encoder layers, mask dim
16, GN, dropout 0; N = 3 frames of maps 12 x 16, 6 x 8, 3 x 4, 1 x 2 (62 encoder tokens; the 1 x 2 level is all border); the
offsets / attention-weight projections randomised as g2_pixel_decoder does; 1-D parameters moved off 0 / 1.  (Maps of 16 x 24 ...
2 x 3 — 126 tokens — were tried first with N = 3, 2 and 1: no seed in 200 met the fixture condition below.  With these projections
the offsets reach 20 pixels, where fp32 rounding of a 64-term projection alone is about 5e-6 pixel, and the largest of that many
coordinates always passed MARGIN / 10.  The maps were shrunk, not the margin, and as little as a seed allowed: stride-4 maps of
12 x 24, 16 x 16 and 8 x 24 found none either, 12 x 16 did.)

Loss: recorded seeded cotangents on mask_features and on the three multi-scale maps, each divided by its number of elements.

Recorded: inputs, state dict, the outputs, the gradients of every parameter and of the four input maps.

Fixture condition: the bilinear gradient jumps where a sampling coordinate crosses an integer.  Every sampling coordinate (pixel
units, both axes, both layers, in range or not) is recorded for an fp32 run (the reference module) and an fp64 run (the package's
module in float64 with the same weights: the reference's forward casts its inputs to float32 and cannot run in float64).  The weight
seed is the first from 1800 on at which the smallest distance of any coordinate of either run to an integer is >= MARGIN = 5e-5
pixel and the largest fp32-vs-fp64 coordinate difference is <= MARGIN / 10.  Both numbers are in `meta`.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ref_import as R    # noqa: E402
import segmenter_train_cases as C    # noqa: E402

OUT = os.path.join(HERE, "g18_pixel_decoder_train{}.npz")
META = dict(conv_dim=64, heads=2, ffn=128, layers=2, mask_dim=16, frames=3, H=48, W=64)
MARGIN = 5e-5


def inputs():
    gen = torch.Generator().manual_seed(1800)
    N, H, W = META["frames"], META["H"], META["W"]
    feats = {k: torch.randn(N, C.CHANS[k], H // C.STRIDES[k], W // C.STRIDES[k], generator=gen) for k in C.CHANS}
    cd = META["conv_dim"]
    cot = {"mask_features": torch.randn(N, META["mask_dim"], H // 4, W // 4, generator=gen)}
    for i, st in enumerate((32, 16, 8)):
        cot[f"ms{i}"] = torch.randn(N, cd, H // st, W // st, generator=gen)
    return feats, cot


def pixels(shapes, loc):
    """(N, Lq, M, L, P, 2) normalised locations of a run -> pixel units, converted in float64 (the conversion adds no rounding of
    its own to an fp32 run's locations)."""
    s = torch.as_tensor(shapes)
    norm = torch.stack([s[:, 1], s[:, 0]], -1).double()[None, None, None, :, None, :]
    return loc.detach().double() * norm - 0.5


def reference_module(seed):
    m = R.ref("mask2former.modeling.pixel_decoder.msdeformattn")
    SS = sys.modules["detectron2.layers"].ShapeSpec
    torch.manual_seed(seed)
    inp = {k: SS(channels=C.CHANS[k], stride=C.STRIDES[k]) for k in C.CHANS}
    pd = m.MSDeformAttnPixelDecoder(
        inp, transformer_dropout=0.0, transformer_nheads=META["heads"], transformer_dim_feedforward=META["ffn"],
        transformer_enc_layers=META["layers"], conv_dim=META["conv_dim"], mask_dim=META["mask_dim"], norm="GN",
        transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    with torch.no_grad():
        for layer in pd.transformer.encoder.layers:         # non-trivial offsets / weights (initialised to 0), as g2_pixel_decoder
            layer.self_attn.sampling_offsets.weight.normal_(0, 0.3)
            layer.self_attn.attention_weights.weight.normal_(0, 0.5)
            layer.self_attn.attention_weights.bias.normal_(0, 0.5)
        for n, p in pd.named_parameters():                  # biases and norms away from 0 / 1: their gradients then test something
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape))
    return pd.train()


def spy_on(module, name, store):
    """Record the sampling coordinates that reach `module.name(value, shapes, loc, w)`."""
    inner = getattr(module, name)

    def spy(value, shapes, loc, w):
        store.append(pixels(shapes.tolist(), loc))
        return inner(value, shapes, loc, w)
    setattr(module, name, spy)
    return lambda: setattr(module, name, inner)


def main():
    for seed in range(1800, 2000):
        try:
            return generate(seed)
        except AssertionError as e:
            if "fixture condition" not in str(e):
                raise
            print("seed", seed, ":", e)
    raise SystemExit("no seed in 200 met the fixture condition: shrink N or the maps, not the margin")


def generate(seed):
    feats, cot = inputs()
    pd = reference_module(seed)
    c32, c64 = [], []
    modm = sys.modules["mask2former.modeling.pixel_decoder.ops.modules.ms_deform_attn"]
    undo = spy_on(modm, "ms_deform_attn_core_pytorch", c32)
    leaves = {k: v.clone().requires_grad_() for k, v in feats.items()}
    mf, out0, ms = pd.forward_features(leaves)
    undo()
    assert len(c32) == META["layers"]
    # the fp64 run: the package's module, float64, the same weights
    from dvis_plus_amd import functions as Fn
    own = C.build_pixel_decoder(META, dtype=torch.float64, state=pd.state_dict()).train()
    undo = spy_on(Fn, "ms_deform_attn_core_pytorch", c64)
    with torch.no_grad():
        mf64, _, ms64 = own.forward_features({k: v.double() for k, v in feats.items()})
    undo()
    assert len(c64) == META["layers"] and mf64.dtype == torch.float64
    dist = min(float((c - c.round()).abs().min()) for c in c32 + c64)
    assert dist >= MARGIN, f"fixture condition: a sampling coordinate {dist:.3e} pixel from an integer (< {MARGIN})"
    diff = max(float((a.double() - b).abs().max()) for a, b in zip(c32, c64))
    assert diff <= MARGIN / 10, f"fixture condition: fp32 and fp64 sampling coordinates differ by {diff:.3e} pixel (> {MARGIN / 10})"
    assert float((mf.double() - mf64).abs().max()) < 1e-4           # the two runs are the same model

    C.g18_loss(mf, ms, cot).backward()
    meta = dict(META, weight_seed=seed, margin=MARGIN, smallest_distance_to_integer=dist, largest_fp32_fp64_coordinate_diff=diff,
                coordinates=int(sum(c.numel() for c in c32)))
    arrays = {f"in/{k}": v.numpy() for k, v in feats.items()}
    arrays.update({f"cot/{k}": v.numpy() for k, v in cot.items()})
    arrays.update({"out/mask_features": mf.detach().numpy(), "out/out0": out0.detach().numpy()})
    arrays.update({f"out/ms{i}": m.detach().numpy() for i, m in enumerate(ms)})
    arrays.update({f"gi/{k}": v.grad.numpy() for k, v in leaves.items()})
    arrays["meta"] = np.array(repr(meta))
    np.savez_compressed(OUT.format(""), **arrays)
    np.savez_compressed(OUT.format("_state"), **{k: v.numpy().copy() for k, v in pd.state_dict().items()})
    grads = {}
    for n, p in pd.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
        grads[n] = p.grad.numpy().copy()
    np.savez_compressed(OUT.format("_grads"), **grads)
    for suffix in ("", "_state", "_grads"):
        size = os.path.getsize(OUT.format(suffix))
        assert size < 1 << 20, (suffix, size)
        print("wrote", OUT.format(suffix), size, "bytes")
    print(meta)


if __name__ == "__main__":
    main()
