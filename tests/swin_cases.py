"""Shared helpers of the Swin tests (test_swin_cpu.py, test_window_attention_gpu.py, test_swin_gpu.py) and of
tests/golden/gen_swin_golden.py: the rule that fills a Swin's weights from one seeded generator (the g21 fixtures store no weights),
the fixtures, the literal roll / pad / partition / mask composition of a Swin block's attention, and the kernel test cases."""
import functools
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("g21_swin_w7", "g21_swin_w12")
# name -> (WINDOW_SIZE, image shape); both: EMBED_DIM 32, DEPTHS [2, 2, 2, 2], NUM_HEADS [1, 2, 4, 8] (head dim 32)
FIXTURE_SPECS = {"g21_swin_w7": (7, (2, 3, 58, 90)),          # token grids 15x23, 8x12, 4x6, 2x3
                 "g21_swin_w12": (12, (1, 3, 64, 150))}       # token grids 16x38, 8x19, 4x10, 2x5
SEED = 2100


def swin_cfg(window_size, embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), **swin):
    """A config node with the reference's MODEL.SWIN defaults and the toy sizes of the fixtures."""
    from dvis_plus_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cfg.MODEL.BACKBONE.NAME = "D2SwinTransformer"
    cfg.MODEL.SWIN.merge({"EMBED_DIM": embed_dim, "DEPTHS": list(depths), "NUM_HEADS": list(num_heads), "WINDOW_SIZE": window_size, **swin})
    return cfg


def fill_weights(module, seed=SEED):
    """THE rule (generator and tests alike): every entry of ``sorted(state_dict())`` from one seeded CPU generator — linear /
    convolution weights randn / sqrt(fan_in); LayerNorm weights 1 + 0.1 randn; biases 0.1 randn except qkv biases 0.5 randn (so that
    pad tokens matter); relative-position bias tables 1.0 randn; the integer ``relative_position_index`` buffers stay."""
    g = torch.Generator().manual_seed(seed)
    sd = module.state_dict()
    new = {}
    for name in sorted(sd):
        t = sd[name]
        if not t.is_floating_point():
            new[name] = t.clone()
            continue
        r = torch.randn(t.shape, generator=g, dtype=torch.float32)
        if name.endswith("relative_position_bias_table"):
            v = r
        elif name.endswith(".weight") and t.dim() == 1:
            v = 1 + 0.1 * r
        elif name.endswith(".weight"):
            v = r / math.sqrt(t[0].numel())
        elif name.endswith("qkv.bias"):
            v = 0.5 * r
        else:
            assert name.endswith(".bias"), name
            v = 0.1 * r
        new[name] = v.to(t.dtype)
    module.load_state_dict(new, strict=True)
    return module


def fixture_image(name):
    ws, shape = FIXTURE_SPECS[name]
    return torch.randn(shape, generator=torch.Generator().manual_seed(SEED + ws), dtype=torch.float32)


class Fixture:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.meta = json.loads(str(z["meta"]))
        self.image = torch.from_numpy(z["image"])
        self.outs = {k: torch.from_numpy(z[k]) for k in z.files if k not in ("meta", "image")}     # res2..res5, block0, block1

    def build(self, device="cpu"):
        """This package's D2SwinTransformer through d2.build_backbone, weights by the rule."""
        from dvis_plus_amd import d2
        m = self.meta["cfg"]
        cfg = swin_cfg(m["WINDOW_SIZE"], m["EMBED_DIM"], m["DEPTHS"], m["NUM_HEADS"])
        return fill_weights(d2.build_backbone(cfg, None), self.meta["seed"]).eval().to(device)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return Fixture(name)


def run_with_blocks(model, image):
    """model(image) under no_grad -> {res2..res5, block0, block1}: stage 1's two block outputs are taken by forward hooks."""
    got, hooks = {}, []
    for i, blk in enumerate(model.layers[0].blocks):
        hooks.append(blk.register_forward_hook(lambda mod, args, out, i=i: got.__setitem__(f"block{i}", out.detach())))
    try:
        with torch.no_grad():
            got.update(model(image))
    finally:
        for h in hooks:
            h.remove()
    return got


# ------------------------------------------------------------------------------------------- the attention of one block, literally
def literal_window_attention(qkv_rows, qkv_bias, table, B, H, W, heads, ws, shift, scale=None):
    """What a Swin block does between norm1 and proj, step by step: view as a map, pad to window multiples (a padded token's qkv is
    the bias: the padding follows norm1 and precedes the projection), roll by -shift, partition, per window and head scale q, q k^T,
    add the gathered relative-position bias, add the 0 / -100 mask built from the nine image regions, softmax, times v, merge the
    windows, roll back, crop.  qkv_rows (B, H W, 3 C) -> (B, H W, C)."""
    C = qkv_rows.shape[-1] // 3
    d, N = C // heads, ws * ws
    scale = d ** -0.5 if scale is None else scale
    x = qkv_rows.view(B, H, W, 3 * C)
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    Hp, Wp = H + pad_b, W + pad_r
    padded = (torch.zeros(3 * C, dtype=x.dtype) if qkv_bias is None else qkv_bias.to(x.dtype)).expand(B, Hp, Wp, 3 * C).clone()
    padded[:, :H, :W] = x
    x = torch.roll(padded, shifts=(-shift, -shift), dims=(1, 2)) if shift > 0 else padded
    part = lambda t: t.view(t.shape[0], Hp // ws, ws, Wp // ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(-1, N, t.shape[-1])
    win = part(x)                                                                        # (B nW, N, 3 C)
    q, k, v = win.reshape(-1, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    attn = (q * scale) @ k.transpose(-2, -1)
    cy, cx = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    cy, cx = cy.flatten(), cx.flatten()
    index = (cy[:, None] - cy[None, :] + ws - 1) * (2 * ws - 1) + (cx[:, None] - cx[None, :] + ws - 1)
    attn = attn + table.to(x.dtype)[index.view(-1)].view(N, N, heads).permute(2, 0, 1).unsqueeze(0)
    if shift > 0:
        img = torch.zeros(1, Hp, Wp, 1, dtype=x.dtype)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[:, hs, wsl, :] = cnt
                cnt += 1
        mw = part(img).view(-1, N)
        mask = mw.unsqueeze(1) - mw.unsqueeze(2)
        mask = mask.masked_fill(mask != 0, -100.0).masked_fill(mask == 0, 0.0)
        nW = mask.shape[0]
        attn = (attn.view(B, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    o = (torch.softmax(attn, dim=-1) @ v).transpose(1, 2).reshape(-1, ws, ws, C)
    o = o.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o[:, :H, :W].reshape(B, H * W, C)


# (H, W, ws, heads, C): the shapes the formulation was checked at against the reference's SwinTransformerBlock
CPU_SHAPES = ((10, 13, 7, 2, 64), (12, 24, 12, 1, 32), (5, 30, 12, 3, 96), (9, 9, 3, 2, 16), (7, 7, 7, 2, 64))

# name -> (H, W, ws, heads, B): the kernel's cases, head dim 32; each runs with shift 0 and ws // 2
KERNEL_CASES = {
    "one window, tile tails": (7, 7, 7, 1, 1),
    "pads on both axes": (10, 13, 7, 2, 2),
    "exact fit": (12, 24, 12, 1, 1),
    "map shorter than a window": (5, 30, 12, 3, 2),
    "more work units than a bounded grid would hold": (64, 100, 7, 1, 3),
}


def attention_inputs(B, H, W, heads, ws, d=32, seed=0, bias=True, table_scale=1.0, qk_scale=1.0):
    g = torch.Generator().manual_seed(2150 + seed)
    C = heads * d
    qkv = torch.randn(B, H * W, 3 * C, generator=g)
    qkv[..., :2 * C] *= qk_scale
    qkv_bias = 0.5 * torch.randn(3 * C, generator=g) if bias else None
    table = table_scale * torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    return qkv, qkv_bias, table


@functools.lru_cache(maxsize=None)
def kernel_case(name, shifted, bias=True, table_scale=1.0, qk_scale=1.0):
    """Seeded inputs of a case and its fp32 / fp64 CPU references (cpu_ops.window_attention), computed once and left unchanged."""
    from dvis_plus_amd import cpu_ops
    H, W, ws, heads, B = KERNEL_CASES[name]
    shift = ws // 2 if shifted else 0
    qkv, qkv_bias, table = attention_inputs(B, H, W, heads, ws, seed=sorted(KERNEL_CASES).index(name), bias=bias,
                                            table_scale=table_scale, qk_scale=qk_scale)
    run = lambda dt: cpu_ops.window_attention(qkv.to(dt), None if qkv_bias is None else qkv_bias.to(dt), table.to(dt), B, H, W, heads, ws,
                                              shift)
    return dict(qkv=qkv, qkv_bias=qkv_bias, table=table, args=(B, H, W, heads, ws, shift), cpu32={"out": run(torch.float32)},
                cpu64={"out": run(torch.float64)})


# ------------------------------------------------------------------------------------------------- toy video models on Swin
def toy_video_cfg(arch="DVIS_Plus_online", window_size=7, T=2):
    """A cfg for `arch` with ``BACKBONE.NAME: D2SwinTransformer`` at toy sizes (64-wide heads of 2 x 32, 8 queries, 5 classes), the
    loss keys included so that from_config builds the criterion."""
    cfg = swin_cfg(window_size)
    cfg.merge({
        "MODEL": {"META_ARCHITECTURE": arch,
                  "SEM_SEG_HEAD": {"NUM_CLASSES": 5, "CONVS_DIM": 64, "MASK_DIM": 64, "TRANSFORMER_ENC_LAYERS": 1},
                  "MASK_FORMER": {"HIDDEN_DIM": 64, "NHEADS": 2, "DIM_FEEDFORWARD": 128, "DEC_LAYERS": 3, "NUM_OBJECT_QUERIES": 8,
                                  "REID_HIDDEN_DIM": 64, "CLASS_WEIGHT": 2.0, "MASK_WEIGHT": 5.0, "DICE_WEIGHT": 5.0,
                                  "TRAIN_NUM_POINTS": 64, "DEEP_SUPERVISION": True, "NO_OBJECT_WEIGHT": 0.1, "OVERSAMPLE_RATIO": 3.0,
                                  "IMPORTANCE_SAMPLE_RATIO": 0.75, "TEST": {"TASK": "vis", "MAX_NUM": 5}},
                  "TRACKER": {"DECODER_LAYERS": 2, "USE_CL": False}},
        "INPUT": {"SAMPLING_FRAME_NUM": T}, "SOLVER": {"MAX_ITER": 2}})
    if arch == "MinVIS":
        cfg.MODEL.MASK_FORMER.TRANSFORMER_DECODER_NAME = "VideoMultiScaleMaskedTransformerDecoder_minvis"
    return cfg


def toy_online_model(device="cpu", seed=21, window_size=7):
    """DVIS_Plus_online from the cfg, seeded; the Swin's weights by the rule, the encoder's offset / attention-weight projections
    randomised (they start at zero weights) as the other toy stages do."""
    from dvis_plus_amd.config import build_model
    torch.manual_seed(seed)
    m = build_model(toy_video_cfg("DVIS_Plus_online", window_size), n_things=5)
    fill_weights(m.backbone)
    with torch.no_grad():
        for layer in m.sem_seg_head.pixel_decoder.transformer.encoder.layers:
            layer.self_attn.sampling_offsets.weight.normal_(0, 0.3)
            layer.self_attn.attention_weights.weight.normal_(0, 0.5)
            layer.self_attn.attention_weights.bias.normal_(0, 0.5)
    return m.eval().to(device)


def toy_video(T=2, H=64, W=96, seed=0, instances=False):
    g = torch.Generator().manual_seed(2170 + seed)
    video = {"image": [torch.rand(3, H, W, generator=g) * 255 for _ in range(T)], "height": H, "width": W}
    if instances:
        from tracker_train_cases import Instances
        inst = []
        for f in range(T):
            masks = torch.zeros(2, H, W, dtype=torch.bool)
            masks[0, 4 + f:H // 2, 6:W // 2] = True
            masks[1, H // 2:, W // 3 + f:] = True
            inst.append(Instances(torch.tensor([0, 1]), torch.tensor([1, 3]), masks))
        video["instances"] = inst
    return video
