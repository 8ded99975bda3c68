"""Swin Transformer backbone (inference; frozen under the tracker / refiner stages) — SURVEY.md row 27.

Mirrors the reference's backbone: same constructor arguments, module tree, ``state_dict()`` keys and shapes (the persistent
``relative_position_index`` buffers included, so its checkpoints load with ``strict=True``) and outputs
  SwinTransformer (+ PatchEmbed, BasicLayer, SwinTransformerBlock, WindowAttention, Mlp, PatchMerging)
                                           mask2former/modeling/backbone/swin.py:21-684
  D2SwinTransformer (detectron2 backbone wrapper: dict res2..res5, keys MODEL.SWIN.*)        .../swin.py:686-770, config.py:74-90

What runs where: a block is ``Fn.add_layer_norm`` -> qkv projection -> ``Fn.window_attention`` -> out-projection with the residual
in its epilogue -> LayerNorm -> fc1 + GELU -> fc2 + residual, the dispatch of the ViT blocks' plain branch (vit_adapter.Block).
``Fn.window_attention`` (csrc/window_attention.hip) takes the qkv rows of the UNPADDED token grid and does F.pad, both torch.roll,
window partition / reverse, the qkv permute, the relative-position-bias gather, the region mask, softmax, both products and the
crop as index arithmetic: neither the (nW, N, N) mask matrix nor the gathered (heads, N, N) bias is ever materialised.  The patch
embedding is a GEMM over (tokens, 3 p p) rows — no library convolution; patch merging is the reference's slicing + LayerNorm +
bias-free projection.  Drop-path, dropout and activation checkpointing have no effect on an evaluation result and are not built.

Training: there is no window-attention backward.  ``forward`` keys off grad mode: with grad enabled and a parameter that requires
grad it raises ``NotImplementedError``; under ``torch.no_grad()`` (how ``DVIS_Plus_online`` / ``DVIS_Plus_offline`` run their frozen
segmenter in ``.train()``) it is the inference forward, whatever ``self.training`` says.
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import functions as Fn
from .registry import BACKBONE_REGISTRY, ShapeSpec


def _layer_norm(x, norm):
    """``Fn.layer_norm``: the fused kernel where it serves the width (C <= 1024: every norm of Swin-T / S / B and all but the last
    stage's of Swin-L), torch's LayerNorm beyond (Swin-L's 1536-wide last stage and its 1536 / 3072-wide merging norms)."""
    return Fn.layer_norm(x, norm)


def patch_tokens(x, proj, norm=None):
    """A stride-p p x p convolution `proj` over (B, Cin, H, W), H and W multiples of p, as a linear layer over flattened patches
    — one gather into (B h w, Cin p p) rows and a GEMM whose output already is the token matrix —, then `norm`:
    -> tokens (B, h w, C), h, w.  Shared by PatchEmbed and the CLIP ConvNeXt stem."""
    ph, pw = proj.kernel_size
    B, Cin, H, W = x.shape
    h, w = H // ph, W // pw
    rows = x.reshape(B, Cin, h, ph, w, pw).permute(0, 2, 4, 1, 3, 5).reshape(B * h * w, Cin * ph * pw)
    t = Fn.linear(rows, proj.weight.view(proj.out_channels, -1), proj.bias, tall=True).view(B, h * w, proj.out_channels)
    return (t if norm is None else Fn.layer_norm(t, norm)), h, w


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)
        self.drop = nn.Dropout(drop)


class WindowAttention(nn.Module):
    """The parameters of W-MSA / SW-MSA (swin.py:74-129); the computation is ``Fn.window_attention`` in the block."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        self.dim, self.window_size, self.num_heads = dim, tuple(window_size), num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        wh, ww = self.window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * wh - 1) * (2 * ww - 1), num_heads))
        # (a persistent buffer of the reference's state dict; the kernel computes the index from the coordinates instead)
        cy, cx = torch.meshgrid(torch.arange(wh), torch.arange(ww), indexing="ij")
        cy, cx = cy.flatten(), cx.flatten()
        index = (cy[:, None] - cy[None, :] + wh - 1) * (2 * ww - 1) + (cx[:, None] - cx[None, :] + ww - 1)
        self.register_buffer("relative_position_index", index)
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        self.softmax = nn.Softmax(dim=-1)


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size=7, shift_size=0, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0,
                 attn_drop=0.0, drop_path=0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim, self.num_heads, self.window_size, self.shift_size, self.mlp_ratio = dim, num_heads, window_size, shift_size, mlp_ratio
        assert 0 <= self.shift_size < self.window_size, "shift_size must in 0-window_size"
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, window_size=(window_size, window_size), num_heads=num_heads, qkv_bias=qkv_bias,
                                    qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def forward(self, x, H, W):
        """x (B, H W, C) -> (B, H W, C) (swin.py:235-295; the mask matrix of the reference's signature is the kernel's arithmetic)."""
        B, L, C = x.shape
        assert L == H * W, "input feature has wrong size"
        a, m = self.attn, self.mlp
        qkv = Fn.linear(_layer_norm(x, self.norm1), a.qkv.weight, a.qkv.bias, tall=True)
        o = Fn.window_attention(qkv.contiguous(), a.qkv.bias, a.relative_position_bias_table, B, H, W, a.num_heads, self.window_size,
                                self.shift_size, a.scale)
        x = Fn.linear(o, a.proj.weight, a.proj.bias, tall=True, residual=x)
        h = Fn.linear(_layer_norm(x, self.norm2), m.fc1.weight, m.fc1.bias, tall=True, act="gelu")      # exact (erf) GELU as nn.GELU()
        return Fn.linear(h, m.fc2.weight, m.fc2.bias, tall=True, residual=x)


class PatchMerging(nn.Module):
    def __init__(self, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def forward(self, x, H, W):
        """swin.py:311-337: an odd map is padded with zero rows, the four 2 x 2 phases are concatenated along the channels."""
        B, L, C = x.shape
        assert L == H * W, "input feature has wrong size"
        x = x.view(B, H, W, C)
        if H % 2 == 1 or W % 2 == 1:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).view(B, -1, 4 * C)
        return Fn.linear(_layer_norm(x, self.norm), self.reduction.weight, None, tall=True)


class BasicLayer(nn.Module):
    def __init__(self, dim, depth, num_heads, window_size=7, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0, attn_drop=0.0,
                 drop_path=0.0, norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False):
        super().__init__()
        self.window_size, self.shift_size, self.depth, self.use_checkpoint = window_size, window_size // 2, depth, use_checkpoint
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, num_heads=num_heads, window_size=window_size, shift_size=0 if i % 2 == 0 else window_size // 2,
                                 mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                                 norm_layer=norm_layer) for i in range(depth)])
        self.downsample = downsample(dim=dim, norm_layer=norm_layer) if downsample is not None else None

    def forward(self, x, H, W):
        for blk in self.blocks:
            x = blk(x, H, W)
        if self.downsample is not None:
            return x, H, W, self.downsample(x, H, W), (H + 1) // 2, (W + 1) // 2
        return x, H, W, x, H, W


class PatchEmbed(nn.Module):
    def __init__(self, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.patch_size = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
        self.in_chans, self.embed_dim = in_chans, embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None

    def forward(self, x):
        """(B, 3, H, W) -> tokens (B, h w, C), h, w (swin.py:479-495 up to the layout: the reference returns the NCHW map and its
        caller flattens it).  The stride-p p x p convolution is a linear layer over flattened patches: one gather into (B h w, 3 p p)
        rows and a GEMM whose output already is the token matrix."""
        ph, pw = self.patch_size
        B, Cin, H, W = x.shape
        if W % pw != 0:
            x = F.pad(x, (0, pw - W % pw))
        if H % ph != 0:
            x = F.pad(x, (0, 0, 0, ph - H % ph))
        return patch_tokens(x, self.proj, self.norm)


class SwinTransformer(nn.Module):
    def __init__(self, pretrain_img_size=224, patch_size=4, in_chans=3, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24),
                 window_size=7, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.2,
                 norm_layer=nn.LayerNorm, ape=False, patch_norm=True, out_indices=(0, 1, 2, 3), frozen_stages=-1, use_checkpoint=False):
        """drop_rate / attn_drop_rate / drop_path_rate / use_checkpoint: accepted, and without effect on an evaluation result."""
        super().__init__()
        if ape:
            raise NotImplementedError("dvis_plus_amd: MODEL.SWIN.APE (the absolute position embedding, bicubically resized per input "
                                      "size) is not built; no yaml of the reference sets it")
        self.pretrain_img_size, self.num_layers, self.embed_dim = pretrain_img_size, len(depths), embed_dim
        self.ape, self.patch_norm, self.out_indices, self.frozen_stages = ape, patch_norm, out_indices, frozen_stages
        self.patch_embed = PatchEmbed(patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      norm_layer=norm_layer if patch_norm else None)
        self.pos_drop = nn.Dropout(p=drop_rate)
        self.layers = nn.ModuleList([
            BasicLayer(dim=int(embed_dim * 2 ** i), depth=depths[i], num_heads=num_heads[i], window_size=window_size, mlp_ratio=mlp_ratio,
                       qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate, norm_layer=norm_layer,
                       downsample=PatchMerging if i < self.num_layers - 1 else None, use_checkpoint=use_checkpoint)
            for i in range(self.num_layers)])
        self.num_features = [int(embed_dim * 2 ** i) for i in range(self.num_layers)]
        for i in out_indices:
            self.add_module(f"norm{i}", norm_layer(self.num_features[i]))
        self._freeze_stages()

    def _freeze_stages(self):
        """swin.py:618-633."""
        if self.frozen_stages >= 0:
            self.patch_embed.eval()
            self.patch_embed.requires_grad_(False)
        if self.frozen_stages >= 2:
            self.pos_drop.eval()
            for i in range(0, self.frozen_stages - 1):
                self.layers[i].eval()
                self.layers[i].requires_grad_(False)

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        return self

    @Fn.fp32_island
    def forward(self, x):
        """(B, 3, H, W) -> {"res2".."res5": (B, C_i, H_i, W_i)} for the stages of out_indices."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("dvis_plus_amd: the Swin backbone does not train: there is no window-attention backward "
                                      "(csrc/window_attention.hip is inference-only).  The tracker and refiner stages "
                                      "(DVIS_Plus_online / DVIS_Plus_offline .train()) run this backbone frozen, under torch.no_grad(); "
                                      "call it there, or freeze it with requires_grad_(False)")
        x = Fn.f32(x) if x.is_cuda else x
        x, Wh, Ww = self.patch_embed(x)
        outs = {}
        for i, layer in enumerate(self.layers):
            x_out, H, W, x, Wh, Ww = layer(x, Wh, Ww)
            if i in self.out_indices:
                x_out = _layer_norm(x_out, getattr(self, f"norm{i}"))
                outs[f"res{i + 2}"] = Fn.tokens_to_map(x_out.contiguous(), 0, H, W).contiguous()
        return outs


@BACKBONE_REGISTRY.register()
class D2SwinTransformer(SwinTransformer):
    """detectron2 backbone surface (swin.py:686-770), built like the reference's: ``D2SwinTransformer(cfg, input_shape)``."""

    def __init__(self, cfg, input_shape=None):
        s = cfg.MODEL.SWIN
        if s.APE:
            raise NotImplementedError("dvis_plus_amd: MODEL.SWIN.APE: True (the absolute position embedding) is not built; no yaml of "
                                      "the reference sets it")
        super().__init__(s.PRETRAIN_IMG_SIZE, s.PATCH_SIZE, 3, s.EMBED_DIM, list(s.DEPTHS), list(s.NUM_HEADS), s.WINDOW_SIZE, s.MLP_RATIO,
                         s.QKV_BIAS, s.QK_SCALE, s.DROP_RATE, s.ATTN_DROP_RATE, s.DROP_PATH_RATE, nn.LayerNorm, s.APE, s.PATCH_NORM,
                         use_checkpoint=s.USE_CHECKPOINT)
        self._out_features = list(s.OUT_FEATURES)
        self._out_feature_strides = {"res2": 4, "res3": 8, "res4": 16, "res5": 32}
        self._out_feature_channels = {f"res{i + 2}": c for i, c in enumerate(self.num_features)}

    def forward(self, x):
        assert x.dim() == 4, f"SwinTransformer takes an input of shape (N, C, H, W). Got {x.shape} instead!"
        y = super().forward(x)
        return {k: v for k, v in y.items() if k in self._out_features}

    def output_shape(self):
        return {name: ShapeSpec(channels=self._out_feature_channels[name], stride=self._out_feature_strides[name])
                for name in self._out_features}

    @property
    def size_divisibility(self):
        return 32
