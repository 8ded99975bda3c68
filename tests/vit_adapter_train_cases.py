"""Shared helpers of the ViT-Adapter training tests (test_dwconv_tokens_backward_gpu.py, test_vit_adapter_train_cpu.py,
test_vit_adapter_train_gpu.py) and of tests/golden/gen_vit_adapter_train_golden.py: the ConvFFN convolution's reference
composition, the g19 fixture (the reference's own DinoV2ViTAdapter in .train() with a frozen ViT) and the MinVIS toy stage with
this backbone."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from segmenter_train_cases import MIN_SAMPLES            # noqa: F401  (the project's rule: below it a tensor is too few samples)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = dict(rtol=2e-3, atol=5e-4)         # tensors of fewer than MIN_SAMPLES elements


# ------------------------------------------------------------------ the token-major depthwise convolution and its reference
def dwconv_composition(x, levels, weight, bias, gelu):
    """adapter.py:83-98 (+ ConvFFN's GELU): per level transpose to NCHW, grouped Conv2d, transpose back; concatenate."""
    B, _, C = x.shape
    outs, off = [], 0
    for h, w in levels:
        m = x[:, off:off + h * w].transpose(1, 2).reshape(B, C, h, w).contiguous()
        outs.append(F.conv2d(m, weight, bias, 1, 1, 1, C).flatten(2).transpose(1, 2))
        off += h * w
    y = torch.cat(outs, dim=1)
    return F.gelu(y) if gelu else y


def dwconv_reference(x, levels, weight, bias, grad_out, gelu, dtype):
    """CPU autograd of the composition in `dtype` -> {"out", "grad_x", "grad_weight"[, "grad_bias"]}."""
    leaves = [t.detach().cpu().to(dtype).requires_grad_() for t in (x, weight) + (() if bias is None else (bias,))]
    y = dwconv_composition(leaves[0], levels, leaves[1], leaves[2] if bias is not None else None, gelu)
    grads = torch.autograd.grad(y, leaves, grad_out.detach().cpu().to(dtype))
    out = {"out": y.detach(), "grad_x": grads[0], "grad_weight": grads[1]}
    if bias is not None:
        out["grad_bias"] = grads[2]
    return out


# name -> (B, C, levels, bias)
DWCONV_CASES = {
    "C4": (1, 4, [(3, 5)], True), "C8": (1, 8, [(3, 5)], True),
    "C260 (crosses the 256-channel workgroup column)": (1, 260, [(3, 5)], True),
    "w1": (1, 8, [(2, 1)], True), "w5": (1, 8, [(2, 5)], True), "w6": (1, 8, [(2, 6)], True), "w7": (1, 8, [(2, 7)], True),
    "w8": (1, 8, [(2, 8)], True),
    "h1": (1, 8, [(1, 6)], True), "h2": (1, 8, [(2, 6)], True), "h3": (1, 8, [(3, 6)], True),
    "stack of (2, 2): all border": (2, 8, [(4, 4), (2, 2), (1, 1)], True),
    "stack of (6, 10)": (1, 16, [(12, 20), (6, 10), (3, 5)], True),
    "B2, batch stride padded beyond the level": (2, 8, [(3, 5), (1, 2)], True),
    "no bias": (1, 8, [(3, 5)], False),
    # 2 x 24 x 44 = 2112 strips = 528 workgroups > the 512 the dz launch is bounded to: the grid-stride loop takes a second turn
    "more strips than the bounded grid": (2, 4, [(24, 176)], True),
}


@functools.lru_cache(maxsize=None)
def dwconv_case(name, gelu):
    """Seeded inputs of a case and its fp32 / fp64 CPU references, computed once and left unchanged."""
    B, C, levels, has_bias = DWCONV_CASES[name]
    g = torch.Generator().manual_seed(1900 + sorted(DWCONV_CASES).index(name))
    N = sum(h * w for h, w in levels)
    x = torch.randn(B, N, C, generator=g)
    weight = torch.randn(C, 1, 3, 3, generator=g) * 0.3
    bias = torch.randn(C, generator=g) if has_bias else None
    grad_out = torch.randn(B, N, C, generator=g)
    cpu32 = dwconv_reference(x, levels, weight, bias, grad_out, gelu, torch.float32)
    cpu64 = dwconv_reference(x, levels, weight, bias, grad_out, gelu, torch.float64)
    return dict(x=x, levels=levels, weight=weight, bias=bias, grad_out=grad_out, cpu32=cpu32, cpu64=cpu64)


def check_4x(got, cpu32, cpu64, what=""):
    """The project's rule: `got` may be 4 x as far from the fp64 CPU run as the fp32 CPU run is wherever a tensor has >= MIN_SAMPLES
    elements; smaller tensors take SMALL.  Prints every figure before it asserts."""
    fails = []
    for n, ref in cpu64.items():
        g = got[n].detach().cpu().double()
        err = (g - ref).abs().max().item()
        if ref.numel() >= MIN_SAMPLES:
            base = (cpu32[n].double() - ref).abs().max().item()
            print(f"{what}{n}: err {err:.3e}, fp32 CPU {base:.3e}, ratio {err / base if base else float('inf'):.2f}")
            if not err <= 4 * base:
                fails.append((n, err, 4 * base))
        else:
            print(f"{what}{n}: err {err:.3e} ({ref.numel()} elements: rtol 2e-3 / atol 5e-4)")
            try:
                torch.testing.assert_close(g, ref, **SMALL)
            except AssertionError as e:
                fails.append((n, err, str(e).splitlines()[0]))
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------- g19
OUTS = ("f1", "f2", "f3", "f4")


def build_adapter(cfg, device="cpu", dtype=torch.float32, state=None, cls=None, **kw):
    """This package's DinoV2ViTAdapter (or the subclass `cls`) at the toy width of g8 / g19 (`cfg` = the fixture's meta["cfg"])."""
    from dvis_plus_amd.vit_adapter import DinoV2ViTAdapter, DinoVisionTransformer
    vit = DinoVisionTransformer(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["embed"], depth=cfg["depth"],
                                num_heads=cfg["heads"], mlp_ratio=4, init_values=0.5, ffn_layer="mlp", block_chunks=0, qkv_bias=True,
                                proj_bias=True, ffn_bias=True)
    kw.setdefault("freeze_backbone", True)
    m = (cls or DinoV2ViTAdapter)(vit_module=vit, pretrain_size=cfg["img_size"], conv_inplane=cfg["conv_inplane"],
                                 n_points=cfg["n_points"],
                                 deform_num_heads=cfg["deform_heads"], init_values=1e-6, interaction_indexes=cfg["interaction_indexes"],
                                 with_cffn=True, cffn_ratio=cfg["cffn_ratio"], deform_ratio=0.5, add_vit_feature=True,
                                 use_extra_extractor=True, **kw)
    if state is not None:
        m.load_state_dict(state, strict=True)
    return m.to(device=device, dtype=dtype)


def g19_loss(outs, cot):
    """Each output contracted with its recorded cotangent, divided by its number of elements."""
    return sum((o * cot[k]).sum() / o.numel() for o, k in zip(outs, OUTS))


def is_bn_buffer(name):
    return name.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked")


class G19:
    def __init__(self):
        load = lambda s: np.load(os.path.join(GOLDEN, f"g19_vit_adapter_train{s}.npz"))
        z = load("")
        self.meta = eval(str(z["meta"]))
        self.x = torch.from_numpy(z["in/x"])
        self.cots = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("cot/")}
        self.outs = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("out/")}
        self.buffers = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("buf/")}
        self.state = {}
        for s in self.meta["state_files"]:
            part = load(s)
            self.state.update({k: torch.from_numpy(part[k]) for k in part.files})
        g = load("_grads")
        self.grads = {k: torch.from_numpy(g[k]) for k in g.files}

    def run(self, device="cpu", dtype=torch.float32):
        """One training forward + backward -> (module, {f1..f4}, {trainable parameter: gradient}, {BatchNorm buffer: value after})."""
        m = build_adapter(self.meta["cfg"], device, dtype, self.state).train()
        outs = m(self.x.to(device=device, dtype=dtype))
        g19_loss(outs, {k: v.to(device=device, dtype=dtype) for k, v in self.cots.items()}).backward()
        grads = {n: p.grad.detach() for n, p in m.named_parameters() if p.requires_grad}
        bufs = {n: b.detach().clone() for n, b in m.named_buffers() if is_bn_buffer(n)}
        return m, dict(zip(OUTS, (o.detach() for o in outs))), grads, bufs


# ------------------------------------------------------------------------------------------------- the MinVIS toy stage
def minvis_vit_model(device="cpu", dtype=torch.float32, seed=19):
    """segmenter_train_cases.minvis_model with the toy-width ViT-Adapter as its backbone (frozen ViT)."""
    import segmenter_train_cases as S
    from conftest import Golden
    from dvis_plus_amd.criterion import VideoSetCriterion
    from dvis_plus_amd.matcher import VideoHungarianMatcher
    from dvis_plus_amd.meta_architecture import MaskFormerHead, MinVIS
    from dvis_plus_amd.pixel_decoder import MSDeformAttnPixelDecoder
    from dvis_plus_amd.registry import ShapeSpec
    from dvis_plus_amd.transformer_decoder import VideoMultiScaleMaskedTransformerDecoder_minvis
    cfg = Golden("g10_window_loop").meta["cfg"]
    K, Q, HID, MD = cfg["K"], cfg["Q"], cfg["hidden"], cfg["mask_dim"]
    torch.manual_seed(seed)
    from dvis_plus_amd.vit_adapter import DinoV2ViTAdapter
    acfg = G19().meta["cfg"]
    shapes = {k: ShapeSpec(channels=acfg["embed"], stride=s) for k, s in (("res2", 4), ("res3", 8), ("res4", 16), ("res5", 32))}

    class ToyD2Adapter(DinoV2ViTAdapter):
        """D2VitAdapterDinoV2's surface (a dict of res2..res5, output_shape) at the toy width."""

        def forward(self, x):
            return dict(zip(shapes, super().forward(x)))

        def output_shape(self):
            return shapes

    bb = build_adapter(acfg, cls=ToyD2Adapter)
    with torch.no_grad():
        for n, p in bb.named_parameters():                      # (as g19: the extractors' projections start at zero weights)
            if n.endswith("sampling_offsets.weight"):
                p.normal_(0, 0.05)
            elif n.endswith("attention_weights.weight") or n.endswith("attention_weights.bias"):
                p.normal_(0, 0.5)
    pd = MSDeformAttnPixelDecoder(shapes, transformer_dropout=0.0, transformer_nheads=cfg["nheads"],
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
        dec_layers=cfg["dec_layers"], pre_norm=False, mask_dim=MD, enforce_input_project=False, num_frames=S.T)
    head = MaskFormerHead(num_classes=K, pixel_decoder=pd, transformer_predictor=pred)
    wd = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    wd.update({f"{k}_{i}": v for i in range(cfg["dec_layers"]) for k, v in list(wd.items())[:3]})
    matcher = VideoHungarianMatcher(num_points=64, cost_class=2.0, cost_mask=5.0, cost_dice=5.0)
    crit = VideoSetCriterion(K, matcher=matcher, weight_dict=wd, eos_coef=0.1, losses=["labels", "masks"], num_points=64,
                             oversample_ratio=3.0, importance_sample_ratio=0.75)
    m = MinVIS(backbone=bb, sem_seg_head=head, num_queries=Q, task="vis", num_frames=S.T, criterion=crit)
    m = m.eval().to(device=device, dtype=dtype)
    crit.float()
    return m, wd
