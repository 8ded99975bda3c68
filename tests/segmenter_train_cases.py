"""Shared helpers of the segmenter-training tests (test_segmenter_train_cpu.py, test_segmenter_train_gpu.py,
test_msda_fused_backward_gpu.py) and of tests/golden/gen_pixel_decoder_train_golden.py: the g18 fixture (the reference's own
MSDeformAttnPixelDecoder in .train()), the torch formulation of the fused MSDeformAttn op, and the MinVIS toy stage."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHANS = dict(res2=8, res3=12, res4=16, res5=20)
STRIDES = dict(res2=4, res3=8, res4=16, res5=32)
MIN_SAMPLES = 256          # tests/test_tracker_train_gpu.py's: below it a tensor's own fp32-vs-fp64 figure is too few samples


# ---------------------------------------------------------------------------------------------------------------- g18
def build_pixel_decoder(meta, device="cpu", dtype=torch.float32, state=None):
    from dvis_plus_amd.pixel_decoder import MSDeformAttnPixelDecoder
    from dvis_plus_amd.registry import ShapeSpec
    inp = {k: ShapeSpec(channels=CHANS[k], stride=STRIDES[k]) for k in CHANS}
    pd = MSDeformAttnPixelDecoder(
        inp, transformer_dropout=0.0, transformer_nheads=meta["heads"], transformer_dim_feedforward=meta["ffn"],
        transformer_enc_layers=meta["layers"], conv_dim=meta["conv_dim"], mask_dim=meta["mask_dim"], norm="GN",
        transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    if state is not None:
        pd.load_state_dict(state, strict=True)
    return pd.to(device=device, dtype=dtype)


def g18_loss(mask_features, ms, cot):
    """Each output contracted with its recorded cotangent, divided by its number of elements."""
    total = (mask_features * cot["mask_features"]).sum() / mask_features.numel()
    for i in range(3):
        total = total + (ms[i] * cot[f"ms{i}"]).sum() / ms[i].numel()
    return total


class G18:
    def __init__(self):
        load = lambda s: np.load(os.path.join(GOLDEN, f"g18_pixel_decoder_train{s}.npz"))
        z = load("")
        self.meta = eval(str(z["meta"]))
        self.feats = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in/")}
        self.cots = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("cot/")}
        self.outs = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("out/")}
        self.grads_in = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("gi/")}
        s = load("_state")
        self.state = {k: torch.from_numpy(s[k]) for k in s.files}
        g = load("_grads")
        self.grads = {k: torch.from_numpy(g[k]) for k in g.files}

    def run(self, device="cpu", dtype=torch.float32, state=None):
        """One training forward + backward -> (module, {output name: tensor}, {parameter / 'in.<map>': gradient})."""
        pd = build_pixel_decoder(self.meta, device, dtype, self.state if state is None else state).train()
        feats = {k: v.clone().to(device=device, dtype=dtype).requires_grad_() for k, v in self.feats.items()}
        cot = {k: v.to(device=device, dtype=dtype) for k, v in self.cots.items()}
        mf, out0, ms = pd.forward_features(feats)
        g18_loss(mf, ms, cot).backward()
        outs = {"mask_features": mf.detach(), "out0": out0.detach(), **{f"ms{i}": m.detach() for i, m in enumerate(ms)}}
        grads = {n: p.grad.detach() for n, p in pd.named_parameters()}
        grads.update({f"in.{k}": v.grad.detach() for k, v in feats.items()})
        return pd, outs, grads

    def golden_grads(self):
        return {**self.grads, **{f"in.{k}": v for k, v in self.grads_in.items()}}


def baselines(cpu32, cpu64):
    """tests/test_decoder_train_gpu.py's scheme: {tensor: max |fp32 CPU - fp64 CPU|}; a tensor of fewer than MIN_SAMPLES elements
    takes the relative error of the large parameters of its own module at its own scale, where that is larger than its own figure."""
    err = {n: (cpu32[n].double() - cpu64[n]).abs().max().item() for n in cpu64}
    scale = {n: cpu64[n].abs().max().item() for n in cpu64}
    out = {}
    for n in cpu64:
        out[n] = err[n]
        if cpu64[n].numel() < MIN_SAMPLES:
            module = n.rsplit(".", 1)[0]
            rel = [err[m] / scale[m] for m in cpu64 if m.rsplit(".", 1)[0] == module and cpu64[m].numel() >= MIN_SAMPLES]
            if rel:
                out[n] = max(err[n], max(rel) * scale[n])
    return out


# ------------------------------------------------------------------------------------- the fused op's torch formulation
def fused_torch(value, shapes, ref, offsets, logits, L, P):
    """softmax, locations and the sampling op as torch ops (what MSDeformAttn's unfused branch computes on the CPU)."""
    from dvis_plus_amd import cpu_ops
    N, S, M, D = value.shape
    Lq = ref.shape[1]
    off = offsets[:, :M * L * P * 2].reshape(N, Lq, M, L, P, 2)
    w = torch.softmax(logits[:, :M * L * P].reshape(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
    norm = torch.stack([shapes[..., 1], shapes[..., 0]], -1).to(value.dtype)
    loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    return cpu_ops.ms_deform_attn_core_pytorch(value, shapes, loc.expand(N, -1, -1, -1, -1, -1), w), loc, w


def fused_torch_grads(value, shapes, ref, offsets, logits, grad_out, L, P, dtype):
    """-> (out, grad_value, grad_offsets, grad_logits) of the torch formulation by CPU autograd in `dtype`."""
    v, o, lg = (t.detach().cpu().to(dtype).requires_grad_() for t in (value, offsets, logits))
    out, _, _ = fused_torch(v, shapes.cpu(), ref.detach().cpu().to(dtype), o, lg, L, P)
    gv, go, gl = torch.autograd.grad(out, (v, o, lg), grad_out.detach().cpu().to(dtype).view_as(out))
    return out.detach(), gv, go, gl


def make_fused_inputs(N, M, D, shapes, Lq, P=4, seed=0, nref=None, spread=2.0, margin=1e-3):
    """Seeded fp32 inputs of the fused op: value, shapes, level starts, reference points (nref, Lq, L, 2) in (0, 1), raw offsets in
    pixels (so samples land up to `spread` pixels from the reference point — outside the maps at the borders), logits, grad_out.
    Every sampling coordinate (pixel units) is kept >= margin from an integer: offending offsets are re-drawn, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    s = torch.as_tensor(shapes, dtype=torch.long)
    lsi = torch.cat((s.new_zeros((1,)), s.prod(1).cumsum(0)[:-1]))
    L, S = len(shapes), int(s.prod(1).sum())
    Lq = S if Lq is None else Lq
    nref = N if nref is None else nref
    value = torch.randn(N, S, M, D, generator=g)
    ref = torch.rand(nref, Lq, L, 2, generator=g) * 1.1 - 0.05
    off = (torch.rand(N, Lq, M, L, P, 2, generator=g) * 2 - 1) * spread
    logits = torch.randn(N * Lq, M * L * P, generator=g)
    grad_out = torch.randn(N, Lq, M * D, generator=g)
    off = redraw_near_integers(off, ref, s, g, spread, margin)
    assert float(coordinate_margin(off, ref, s)) >= margin
    return value, s, lsi, ref, off.reshape(N * Lq, M * L * P * 2).contiguous(), logits, grad_out


def pixel_coordinates(off, ref, s):
    """(N, Lq, M, L, P, 2) raw offsets -> sampling coordinates in pixel units (x, y), as the kernels form them."""
    norm = torch.stack([s[:, 1], s[:, 0]], -1).to(off.dtype)[None, None, None, :, None, :]
    return (ref[:, :, None, :, None, :] + off / norm) * norm - 0.5


def coordinate_margin(off, ref, s):
    c = pixel_coordinates(off, ref, s)
    return (c - c.round()).abs().min()


def redraw_near_integers(off, ref, s, g, spread, margin):
    for _ in range(100):
        c = pixel_coordinates(off, ref, s)
        bad = (c - c.round()).abs() < margin
        if not bool(bad.any()):
            return off
        off = torch.where(bad, (torch.rand(off.shape, generator=g) * 2 - 1) * spread, off)
    raise AssertionError("could not move the sampling coordinates off the integers")


# ------------------------------------------------------------------------------------------------- the MinVIS toy stage
T, VIDEOS, H, W = 2, 2, 64, 96


def minvis_model(device="cpu", dtype=torch.float32, seed=18, criterion=True):
    """Toy backbone, the g10-sized head (hidden 32, 1 head, d = 32: the fused op's domain) with the `_minvis` decoder, seeded
    init; the offset / attention-weight projections randomised (their weights start at 0).  -> (model in .eval(), weight_dict)"""
    from conftest import Golden
    from toy_backbone import ToyBackbone
    from dvis_plus_amd.criterion import VideoSetCriterion
    from dvis_plus_amd.matcher import VideoHungarianMatcher
    from dvis_plus_amd.meta_architecture import MaskFormerHead, MinVIS
    from dvis_plus_amd.pixel_decoder import MSDeformAttnPixelDecoder
    from dvis_plus_amd.transformer_decoder import VideoMultiScaleMaskedTransformerDecoder_minvis
    cfg = Golden("g10_window_loop").meta["cfg"]
    K, Q, HID, MD = cfg["K"], cfg["Q"], cfg["hidden"], cfg["mask_dim"]
    torch.manual_seed(seed)
    bb = ToyBackbone()
    pd = MSDeformAttnPixelDecoder(bb.output_shape(), transformer_dropout=0.0, transformer_nheads=cfg["nheads"],
                                  transformer_dim_feedforward=cfg["enc_ffn"], transformer_enc_layers=cfg["enc_layers"],
                                  conv_dim=HID, mask_dim=MD, norm="GN", transformer_in_features=["res3", "res4", "res5"],
                                  common_stride=4)
    with torch.no_grad():
        for layer in pd.transformer.encoder.layers:
            layer.self_attn.sampling_offsets.weight.normal_(0, 0.3)
            layer.self_attn.attention_weights.weight.normal_(0, 0.5)
            layer.self_attn.attention_weights.bias.normal_(0, 0.5)
    pred = VideoMultiScaleMaskedTransformerDecoder_minvis(
        HID, True, num_classes=K, hidden_dim=HID, num_queries=Q, nheads=cfg["nheads"], dim_feedforward=cfg["dec_ffn"],
        dec_layers=cfg["dec_layers"], pre_norm=False, mask_dim=MD, enforce_input_project=False, num_frames=T)
    head = MaskFormerHead(num_classes=K, pixel_decoder=pd, transformer_predictor=pred)
    wd = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    wd.update({f"{k}_{i}": v for i in range(cfg["dec_layers"]) for k, v in list(wd.items())[:3]})
    crit = None
    if criterion:
        matcher = VideoHungarianMatcher(num_points=64, cost_class=2.0, cost_mask=5.0, cost_dice=5.0)
        crit = VideoSetCriterion(K, matcher=matcher, weight_dict=wd, eos_coef=0.1, losses=["labels", "masks"], num_points=64,
                                 oversample_ratio=3.0, importance_sample_ratio=0.75)
    m = MinVIS(backbone=bb, sem_seg_head=head, num_queries=Q, task="vis", num_frames=T, criterion=crit)
    m = m.eval().to(device=device, dtype=dtype)
    if crit is not None:
        crit.float()            # the criterion computes in float32 whatever it is handed (criterion.py), as in the fp64 yardsticks of the other stages
    return m, wd


def minvis_batch(device="cpu"):
    """2 videos x 2 frames with targets as refiner_train_cases.offline_model: 3 instances; the last is absent (id -1) in every
    frame and must be dropped, the second is absent in frame 0; frame 1 hands its masks over as an object with `.tensor`."""
    from tracker_train_cases import BitMasks, Instances
    g = torch.Generator().manual_seed(181)
    batch = []
    for v in range(VIDEOS):
        frames = [(torch.rand(3, H, W, generator=g) * 255).to(device) for _ in range(T)]
        instances = []
        for f in range(T):
            masks = torch.zeros(3, H, W, dtype=torch.bool)
            masks[0, 2 + f + 4 * v:H // 2, 3:W // 2] = True
            masks[1, H // 2:, W // 3 + f:] = f > 0
            ids = torch.tensor([0, 1 if f > 0 else -1, -1])
            instances.append(Instances(ids, torch.tensor([1, 3, 2]), BitMasks(masks) if f == 1 else masks))
        batch.append({"image": frames, "instances": instances, "height": H, "width": W})
    return batch


def spy_matcher(model):
    """Record the matcher's pairs of every call -> list of [(rows, cols), ...] on the CPU."""
    calls, inner = [], model.criterion.matcher.forward

    def forward(outputs, targets, *a, **k):
        idx = inner(outputs, targets, *a, **k)
        calls.append([(torch.as_tensor(r).cpu(), torch.as_tensor(c).cpu()) for r, c in idx])
        return idx
    model.criterion.matcher.forward = forward
    return calls
