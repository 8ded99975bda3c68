"""CLIP ConvNeXt backbone of the open-vocabulary family (inference; frozen in every reference config) — SURVEY.md row 29.

  CLIP (detectron2 backbone wrapper around an open_clip model)                       ov_dvis/backbones/clip.py:26-233
  the open_clip model itself (``open_clip.create_model_and_transforms``: a timm ConvNeXt trunk + projection head, and the text
  transformer) is NOT in the reference tree and neither open_clip nor timm is a dependency here: the module tree below is written
  from their published definitions (timm ``ConvNeXt`` / ``ConvNeXtStage`` / ``ConvNeXtBlock``, open_clip ``TimmModel`` / ``CLIP``).
  Its state-dict keys and the model table are UNVERIFIED against a real ``laion2b_s29b_b131k_ft_soup`` checkpoint;
  they are pinned by tests/golden/ref_state_shapes_clip_convnext.json.

What runs where.  The activation stays token-major (B, h w, C) through a stage.  The stem is a gather of 4 x 4 patches + a GEMM + the
fused LayerNorm; a downsample is the fused LayerNorm + a 2 x 2 patch gather + a GEMM; a block is
  ``Fn.dwconv7x7_ln_tokens`` (csrc/dwconv_ln.hip: conv_dw + permute + norm in one kernel)
  -> ``Fn.linear(fc1, tall=True, act="gelu")`` -> ``Fn.linear(fc2', tall=True, residual=x)``
with the layer scale folded into fc2' = (gamma[:, None] W, gamma b), held in a ``derived.Derived`` of the block (a weight update
refreshes it in place, so captured graphs keep their pointers).  The tall GEMMs take the split-f16 kernels under the same range guard
as Swin and the ViT; ``Fn.x3_disabled()`` gives the exact-fp32 path through the same modules.  Each stage's output is also returned
as the contiguous NCHW map the pixel decoder reads (one tiled transpose per stage); ``clip_vis_dense`` is ``res5`` (``norm_pre`` is an
identity).  LayerNorms outside the blocks use ``Fn.add_layer_norm`` up to C = 1024 and torch's beyond (only the large model's
1536-wide ``head.norm``, on Q rows per frame).

The text tower runs once per vocabulary (the open-vocabulary meta-architectures cache its result): projections through ``Fn.linear``, the 77 x 77
causal attention as the plain torch formulation ``cpu_ops.causal_self_attention``.  The tokenizer (a BPE table) is not built:
``CLIP.text_tokenizer`` is None until the integrator assigns one.  Nothing is downloaded: weights come
from ``load_state_dict``.
"""
import collections
import math

import torch
import torch.nn.functional as F
from torch import nn

from . import cpu_ops, derived, functions as Fn
from .registry import BACKBONE_REGISTRY, ShapeSpec
from .swin import patch_tokens

_CONTEXT, _VOCAB = 77, 49408
# open_clip model configs (timm_model_name convnext_base / convnext_large, timm_proj, embed_dim, text_cfg) — from memory, see above
CLIP_MODELS = {
    "convnext_base_w": dict(dims=(128, 256, 512, 1024), depths=(3, 3, 27, 3), embed=640, head="linear", text=(640, 10, 12)),
    "convnext_base_w_320": dict(dims=(128, 256, 512, 1024), depths=(3, 3, 27, 3), embed=640, head="linear", text=(640, 10, 12)),
    "convnext_large_d": dict(dims=(192, 384, 768, 1536), depths=(3, 3, 27, 3), embed=768, head="mlp", text=(768, 12, 16)),
    "convnext_large_d_320": dict(dims=(192, 384, 768, 1536), depths=(3, 3, 27, 3), embed=768, head="mlp", text=(768, 12, 16)),
}


def clip_model_config(name):
    """The table row of MODEL.FC_CLIP.CLIP_MODEL_NAME (+ context length and vocabulary); models that are not built raise."""
    key = name.lower()
    if key in CLIP_MODELS:
        return dict(CLIP_MODELS[key], context=_CONTEXT, vocab=_VOCAB)
    if "convnext_xxlarge" in key:
        why = "its 3072-wide last stage is beyond the 1536 channels csrc/dwconv_ln.hip serves"
    elif key.replace("-quickgelu", "").startswith("rn"):
        why = "the ResNet CLIP models pool through an attention head (visual_prediction_forward_resnet), which is another feature"
    else:
        why = f"served: {', '.join(sorted(CLIP_MODELS))}"
    raise NotImplementedError(f"dvis_plus_amd: MODEL.FC_CLIP.CLIP_MODEL_NAME: {name!r} is not built ({why})")


class Mlp(nn.Module):
    def __init__(self, dim, hidden, out=None, bias=(True, True)):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden, bias=bias[0])
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, out or dim, bias=bias[1])


class ConvNeXtBlock(nn.Module):
    """timm ConvNeXtBlock (conv_mlp=False): x + gamma * fc2(gelu(fc1(norm(conv_dw(x)))))."""

    def __init__(self, dim, ls_init_value=1e-6):
        super().__init__()
        self.conv_dw = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim, 4 * dim)
        self.gamma = nn.Parameter(ls_init_value * torch.ones(dim))
        self._fc2_scaled = derived.Derived()

    def fc2_scaled(self):
        """(gamma[:, None] W2, gamma b2): the layer scale folded into the second projection, refreshed when any of the three changes."""
        g, fc2 = self.gamma, self.mlp.fc2
        return self._fc2_scaled.get((g, fc2.weight, fc2.bias),
                                    lambda: ((g.detach()[:, None] * fc2.weight.detach()).contiguous(), g.detach() * fc2.bias.detach()))

    def forward(self, x, h, w):
        """x (B, h w, C) -> (B, h w, C)."""
        y = Fn.dwconv7x7_ln_tokens(x, self.conv_dw, self.norm, hw=(h, w))
        y = Fn.linear(y, self.mlp.fc1.weight, self.mlp.fc1.bias, tall=True, act="gelu")              # exact (erf) GELU as nn.GELU()
        w2, b2 = self.fc2_scaled()
        return Fn.linear(y, w2, b2, tall=True, residual=x)


class ConvNeXtStage(nn.Module):
    def __init__(self, in_dim, dim, depth, downsample):
        super().__init__()
        self.downsample = nn.Sequential(nn.LayerNorm(in_dim, eps=1e-6), nn.Conv2d(in_dim, dim, 2, stride=2)) if downsample \
            else nn.Identity()
        self.blocks = nn.Sequential(*[ConvNeXtBlock(dim) for _ in range(depth)])
        self._down_weight = derived.Derived()

    def forward(self, x, h, w):
        """x (B, h w, C_in) -> (tokens (B, h' w', C), h', w').  The 2 x 2 / stride 2 convolution is a GEMM over (ky, kx, c) patch rows
        (an odd map loses its last row / column, as under the convolution) with the weight permuted to that order once."""
        if not isinstance(self.downsample, nn.Identity):
            norm, conv = self.downsample[0], self.downsample[1]
            B, _, C = x.shape
            x = Fn.layer_norm(x, norm)
            h2, w2 = h // 2, w // 2
            rows = x.view(B, h, w, C)[:, :2 * h2, :2 * w2].reshape(B, h2, 2, w2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, h2 * w2, 4 * C)
            wt = self._down_weight.get((conv.weight,), lambda: conv.weight.detach().permute(0, 2, 3, 1).reshape(conv.out_channels, 4 * C)
                                       .contiguous())
            x, h, w = Fn.linear(rows, wt, conv.bias, tall=True), h2, w2
        for blk in self.blocks:
            x = blk(x, h, w)
        return x, h, w


class _TrunkHead(nn.Module):
    """timm's NormMlpClassifierHead with num_classes = 0: global pool (an identity on the 1 x 1 maps it gets here), norm, flatten."""

    def __init__(self, dim):
        super().__init__()
        self.norm = nn.LayerNorm(dim, eps=1e-6)

    def forward(self, x):
        return Fn.layer_norm(x, self.norm)


class ConvNeXtTrunk(nn.Module):
    def __init__(self, dims, depths, in_chans=3):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(in_chans, dims[0], 4, stride=4), nn.LayerNorm(dims[0], eps=1e-6))
        self.stages = nn.Sequential(*[ConvNeXtStage(dims[max(i - 1, 0)], dims[i], depths[i], downsample=i > 0) for i in range(4)])
        self.norm_pre = nn.Identity()
        self.head = _TrunkHead(dims[-1])

    def stem_tokens(self, x):
        """(B, 3, H, W) -> tokens (B, h w, C0), h, w: swin.patch_tokens (gather + GEMM + LayerNorm) on the frame cropped to whole 4 x 4
        patches — the un-padded stride-4 convolution drops a ragged last row / column."""
        H, W = x.shape[-2:]
        return patch_tokens(x[:, :, :H // 4 * 4, :W // 4 * 4], self.stem[0], self.stem[1])

    @Fn.fp32_island
    def forward(self, x):
        """(B, 3, H, W) -> {"stem", "res2" .. "res5": contiguous NCHW maps} (clip.py:117-127)."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("dvis_plus_amd: the CLIP ConvNeXt trunk does not train: csrc/dwconv_ln.hip is inference-only and "
                                      "every reference config freezes it; call it under torch.no_grad(), or freeze it with "
                                      "requires_grad_(False)")
        x = Fn.f32(x) if x.is_cuda else x
        t, h, w = self.stem_tokens(x)
        out = {"stem": Fn.tokens_to_map(t.contiguous(), 0, h, w).contiguous()}
        for i, stage in enumerate(self.stages):
            t, h, w = stage(t, h, w)
            out[f"res{i + 2}"] = Fn.tokens_to_map(t.contiguous(), 0, h, w).contiguous()
        return out


class TimmModel(nn.Module):
    """open_clip's TimmModel with pool = '': the trunk, then ``head`` = proj (linear, no bias) or mlp (fc1 + GELU + bias-free fc2)."""

    def __init__(self, dims, depths, embed, head):
        super().__init__()
        self.trunk = ConvNeXtTrunk(dims, depths)
        if head == "linear":
            self.head = nn.Sequential(collections.OrderedDict(drop=nn.Dropout(0.0), proj=nn.Linear(dims[-1], embed, bias=False)))
        elif head == "mlp":
            self.head = nn.Sequential(collections.OrderedDict(mlp=Mlp(dims[-1], 2 * embed, embed, bias=(True, False))))
        else:
            raise ValueError(f"timm_proj {head!r}: 'linear' or 'mlp'")

    def project(self, x):
        """(..., C3) pooled and normalised features -> (..., embed)."""
        if hasattr(self.head, "proj"):
            return Fn.linear(x, self.head.proj.weight, None)
        m = self.head.mlp
        return Fn.linear(Fn.linear(x, m.fc1.weight, m.fc1.bias, act="gelu"), m.fc2.weight, None)


class ResidualAttentionBlock(nn.Module):
    def __init__(self, width, heads):
        super().__init__()
        self.ln_1 = nn.LayerNorm(width)
        self.attn = nn.MultiheadAttention(width, heads)        # the parameters; the computation is forward() below
        self.ln_2 = nn.LayerNorm(width)
        self.mlp = nn.Sequential(collections.OrderedDict(c_fc=nn.Linear(width, 4 * width), gelu=nn.GELU(),
                                                         c_proj=nn.Linear(4 * width, width)))

    def forward(self, x, attn_mask):
        """x (N, L, D), batch first."""
        a = self.attn
        qkv = Fn.linear(Fn.layer_norm(x, self.ln_1), a.in_proj_weight, a.in_proj_bias)
        x = Fn.linear(cpu_ops.causal_self_attention(qkv, a.num_heads, attn_mask), a.out_proj.weight, a.out_proj.bias, residual=x)
        y = Fn.linear(Fn.layer_norm(x, self.ln_2), self.mlp.c_fc.weight, self.mlp.c_fc.bias, act="gelu")
        return Fn.linear(y, self.mlp.c_proj.weight, self.mlp.c_proj.bias, residual=x)


class TextTransformer(nn.Module):
    def __init__(self, width, heads, layers):
        super().__init__()
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(width, heads) for _ in range(layers)])


class CLIPModel(nn.Module):
    """open_clip's CLIP with a timm visual tower: ``visual``, and the text tower's members directly on the model."""

    def __init__(self, dims, depths, embed, head, text, context=_CONTEXT, vocab=_VOCAB):
        super().__init__()
        width, heads, layers = text
        self.visual = TimmModel(dims, depths, embed, head)
        self.transformer = TextTransformer(width, heads, layers)
        self.token_embedding = nn.Embedding(vocab, width)
        self.positional_embedding = nn.Parameter(torch.empty(context, width))
        self.ln_final = nn.LayerNorm(width)
        self.text_projection = nn.Parameter(torch.empty(width, embed))
        self.logit_scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))
        self.register_buffer("attn_mask", torch.full((context, context), float("-inf")).triu_(1), persistent=False)
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        nn.init.normal_(self.text_projection, std=width ** -0.5)


@BACKBONE_REGISTRY.register()
class CLIP(nn.Module):
    """The reference's CLIP backbone (clip.py:26-233) for the ConvNeXt models of ``CLIP_MODELS``.  ``model_cfg`` (a row of that table
    with ``context`` and ``vocab``) overrides the lookup by name: toy models of the tests."""

    def __init__(self, cfg, input_shape=None, model_cfg=None):
        super().__init__()
        self.model_name = cfg.MODEL.FC_CLIP.CLIP_MODEL_NAME
        self.pretrained = cfg.MODEL.FC_CLIP.CLIP_PRETRAINED_WEIGHTS          # recorded; nothing is downloaded
        mc = dict(model_cfg) if model_cfg is not None else clip_model_config(self.model_name)
        self.model_type = "convnext"
        self.clip_model = CLIPModel(mc["dims"], mc["depths"], mc["embed"], mc["head"], mc["text"], mc.get("context", _CONTEXT),
                                    mc.get("vocab", _VOCAB))
        self.text_tokenizer = None
        d = tuple(mc["dims"])
        self.output_channels = [d[0], *d]
        self._out_feature_strides = {"stem": 2, "res2": 4, "res3": 8, "res4": 16, "res5": 32, "clip_embedding": -1}      # (clip.py:64-71)
        self._out_feature_channels = {"stem": d[0], "res2": d[0], "res3": d[1], "res4": d[2], "res5": d[3],
                                      "clip_embedding": self.dim_latent}
        self.eval()
        self.freeze_everything()

    def freeze_everything(self):
        for param in self.clip_model.parameters():
            param.requires_grad = False

    @Fn.fp32_island
    def encode_text(self, text, normalize=False):
        """Token ids (N, L <= context) -> (N, embed): the features at each row's highest token id (the end-of-text token)."""
        m = self.clip_model
        x = m.token_embedding(text) + m.positional_embedding[:text.shape[1]]
        mask = m.attn_mask[:text.shape[1], :text.shape[1]]
        for blk in m.transformer.resblocks:
            x = blk(x, mask)
        x = Fn.layer_norm(x, m.ln_final)
        x = Fn.linear(x[torch.arange(x.shape[0], device=x.device), text.argmax(dim=-1)].contiguous(), m.text_projection.t())
        return F.normalize(x, dim=-1) if normalize else x

    def tokenize_text(self, text):
        if self.text_tokenizer is None:
            raise RuntimeError("dvis_plus_amd: CLIP.text_tokenizer is not set: the BPE tokenizer is not part of this package.  Assign one "
                               "(e.g. backbone.text_tokenizer = open_clip.get_tokenizer(backbone.model_name)), or hand precomputed "
                               "text embeddings to MinVIS_OV.set_text_classifier (INTEGRATION.md section 18)")
        return self.text_tokenizer(text)

    def extract_features(self, x):
        out = self.clip_model.visual.trunk(x)
        out["clip_vis_dense"] = out["res5"]                               # norm_pre is an identity
        return out

    @Fn.fp32_island
    def visual_prediction_forward(self, x, masks=None):
        """Mask-pooled CLIP features (B, Q, C3) -> (B, Q, embed): trunk.head (its norm), then visual.head (clip.py:147-152)."""
        v = self.clip_model.visual
        return v.project(v.trunk.head(x.contiguous()))

    def get_text_classifier(self, text_list, device):
        self.eval()
        with torch.no_grad():
            return self.encode_text(self.tokenize_text(text_list).to(device), normalize=False)      # un-normalised, as the reference's

    def forward(self, x):
        self.eval()
        with torch.no_grad():
            return self.extract_features(x)

    @property
    def dim_latent(self):
        return self.clip_model.text_projection.shape[-1]

    def output_shape(self):
        return {name: ShapeSpec(channels=self._out_feature_channels[name], stride=self._out_feature_strides[name])
                for name in ["stem", "res2", "res3", "res4", "res5", "clip_embedding"]}

    @property
    def size_divisibility(self):
        return -1
