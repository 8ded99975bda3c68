"""Shared cases of the ConvNeXt / CLIP tests (test_dwconv_ln_gpu.py, test_convnext_cpu.py, test_convnext_gpu.py): the LITERAL torch
composition the package's fused path is compared with.  Nothing here imports dvis_plus_amd: the depthwise convolution is
``F.conv2d(groups=C)`` on NCHW, the block norm a ``permute`` + ``F.layer_norm``, the MLP ``F.linear`` / ``F.gelu``, the layer scale
``gamma * ...``, the text tower ``nn.MultiheadAttention`` under the causal mask — timm's ConvNeXt and open_clip's CLIP as published,
with their state-dict keys, so that one state dict drives both sides."""
import math

import torch
import torch.nn.functional as F
from torch import nn

# (B, h, w, C) of tests/test_dwconv_ln_gpu.py
DWCONV_LN_SHAPES = {
    "1x1 map: every tap but the centre is padding": (1, 1, 1, 8),
    "map smaller than the filter": (2, 3, 5, 8),
    "7x7": (1, 7, 7, 16),
    "odd sizes, C no multiple of a wave's 256": (2, 9, 13, 100),
    "row longer than any x-run, partial last run": (1, 4, 70, 192),
    "C768": (1, 5, 6, 768),
    "C1536: the widest reduction": (2, 4, 5, 1536),
}
EPS = 1e-6


def dwconv_ln_inputs(B, h, w, C, seed=0, bias=True):
    """x (B, h, w, C) = s_c (50 + noise): channel scales s_c spread log-uniformly over 1e-3 .. 1e3, a mean offset of 50 noise widths;
    a (C, 1, 7, 7) filter with positive-mean taps and the inverse channel scale (a trained block's filters undo its input's scales), so
    that every channel of the convolution's result sits near 50 with a spread of a few units — the regime in which E[z^2] - mean^2
    cancels (see test_convnext_cpu.py) —, a conv bias, LayerNorm weight / bias."""
    g = torch.Generator().manual_seed(1000 + seed)
    scale = 10.0 ** (torch.rand(C, generator=g, dtype=torch.float64) * 6 - 3)
    x = (torch.randn(B, h, w, C, generator=g, dtype=torch.float64) + 50.0) * scale
    weight = (torch.randn(C, 1, 7, 7, generator=g, dtype=torch.float64) * 0.25 + 1.0) / 49.0 / scale[:, None, None, None]
    cb = torch.randn(C, generator=g, dtype=torch.float64) * 0.1 if bias else None
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    return dict(x=x, weight=weight, bias=cb, gamma=gamma, beta=beta)


def dwconv_ln_literal(x, weight, bias, gamma, beta, eps=EPS):
    """ConvNeXtBlock up to mlp.fc1 as torch runs it: NCHW grouped convolution, permute to NHWC, layer_norm.  x (B, h, w, C)."""
    C = x.shape[-1]
    z = F.conv2d(x.permute(0, 3, 1, 2), weight, bias, stride=1, padding=3, groups=C)
    return F.layer_norm(z.permute(0, 2, 3, 1), (C,), gamma, beta, eps)


def dwconv_ln_shortcut(x, weight, bias, gamma, beta, eps=EPS):
    """The same with the variance taken as E[z^2] - mean^2 (what the kernel must NOT do), in x's dtype."""
    C = x.shape[-1]
    z = F.conv2d(x.permute(0, 3, 1, 2), weight, bias, stride=1, padding=3, groups=C).permute(0, 2, 3, 1)
    mean = z.mean(-1, keepdim=True)
    var = (z * z).mean(-1, keepdim=True) - mean * mean
    return (z - mean) * torch.rsqrt(var + eps) * gamma + beta


def cast(d, dtype):
    return {k: (None if v is None else v.to(dtype)) for k, v in d.items()}


def check_dwconv_ln_refusals(lib, ctypes):
    """dvis_dwconv7x7_ln_tokens through the C ABI with fake pointers: what it does not serve is refused before the launch (the pointers
    are never read), naming the value; dvis_dwconv7x7_ln_tokens_supported agrees.  `lib`: the loaded library (the caller's import)."""
    def call(x=4096, out=1 << 20, stride=3 * 5 * 8, B=1, h=3, w=5, C=8, weight=8192, bias=8192 + 4096, gamma=16384, beta=16384 + 4096):
        p = lambda v: None if v is None else ctypes.c_void_p(v)
        rc = lib.dvis_dwconv7x7_ln_tokens(p(x), p(out), stride, B, h, w, C, p(weight), p(bias), p(gamma), p(beta), 1e-6, None)
        return rc, lib.dvis_last_error().decode()

    for C in (8, 12, 100, 192, 768, 1024, 1536):
        assert lib.dvis_dwconv7x7_ln_tokens_supported(C) == 1, C
    for C in (0, 4, 6, 10, 1538, 1540, 3072):
        assert lib.dvis_dwconv7x7_ln_tokens_supported(C) == 0, C
        rc, msg = call(C=C, stride=3 * 5 * C)
        assert rc != 0 and f"C={C}" in msg, (rc, msg)
    rc, msg = call(x=4096 + 4)
    assert rc != 0 and "16-byte aligned" in msg and hex(4096 + 4) in msg, (rc, msg)
    rc, msg = call(out=4096)                                                                      # out is x
    assert rc != 0 and "overlaps" in msg, (rc, msg)
    rc, msg = call(out=4096 + 16 * 8, B=2)                                                        # out starts inside x's second frame
    assert rc != 0 and "overlaps" in msg, (rc, msg)
    rc, msg = call(stride=3 * 5 * 8 - 4)
    assert rc != 0 and f"batch_stride={3 * 5 * 8 - 4}" in msg, (rc, msg)
    rc, msg = call(stride=3 * 5 * 8 + 2)
    assert rc != 0 and f"batch_stride={3 * 5 * 8 + 2}" in msg, (rc, msg)
    rc, msg = call(h=1 << 14, w=1 << 14, stride=(1 << 28) * 8)
    assert rc != 0 and "2^31" in msg, (rc, msg)
    rc, msg = call(B=0)                                                                           # nothing to do: accepted, nothing launched
    assert rc == 0, (rc, msg)


# ------------------------------------------------------------------------------------------ the literal CLIP ConvNeXt (timm / open_clip)
class LayerNorm2d(nn.LayerNorm):
    """timm's LayerNorm2d: LayerNorm over the channels of an NCHW map."""

    def forward(self, x):
        return F.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias, self.eps).permute(0, 3, 1, 2)


class LitMlp(nn.Module):
    def __init__(self, dim, hidden, out=None, bias=(True, True)):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden, bias=bias[0])
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, out or dim, bias=bias[1])

    def forward(self, x):
        return F.linear(F.gelu(F.linear(x, self.fc1.weight, self.fc1.bias)), self.fc2.weight, self.fc2.bias)


class LitBlock(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.conv_dw = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = LitMlp(dim, 4 * dim)
        self.gamma = nn.Parameter(1e-6 * torch.ones(dim))

    def forward(self, x):
        shortcut = x
        x = F.conv2d(x, self.conv_dw.weight, self.conv_dw.bias, padding=3, groups=x.shape[1])
        x = x.permute(0, 2, 3, 1)
        x = F.layer_norm(x, (x.shape[-1],), self.norm.weight, self.norm.bias, self.norm.eps)
        x = self.mlp(x)
        x = x.permute(0, 3, 1, 2)
        x = self.gamma.reshape(1, -1, 1, 1) * x
        return x + shortcut


class LitStage(nn.Module):
    def __init__(self, in_dim, dim, depth, downsample):
        super().__init__()
        self.downsample = nn.Sequential(LayerNorm2d(in_dim, eps=1e-6), nn.Conv2d(in_dim, dim, 2, stride=2)) if downsample else nn.Identity()
        self.blocks = nn.Sequential(*[LitBlock(dim) for _ in range(depth)])

    def forward(self, x):
        return self.blocks(self.downsample(x))


class LitTrunkHead(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.global_pool = nn.AdaptiveAvgPool2d(1)
        self.norm = LayerNorm2d(dim, eps=1e-6)
        self.flatten = nn.Flatten(1)

    def forward(self, x):
        return self.flatten(self.norm(self.global_pool(x)))


class LitTrunk(nn.Module):
    def __init__(self, dims, depths):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, dims[0], 4, stride=4), LayerNorm2d(dims[0], eps=1e-6))
        self.stages = nn.Sequential(*[LitStage(dims[max(i - 1, 0)], dims[i], depths[i], i > 0) for i in range(4)])
        self.norm_pre = nn.Identity()
        self.head = LitTrunkHead(dims[-1])


class LitVisual(nn.Module):
    def __init__(self, dims, depths, embed, head):
        super().__init__()
        import collections
        self.trunk = LitTrunk(dims, depths)
        if head == "linear":
            self.head = nn.Sequential(collections.OrderedDict(drop=nn.Dropout(0.0), proj=nn.Linear(dims[-1], embed, bias=False)))
        else:
            self.head = nn.Sequential(collections.OrderedDict(mlp=LitMlp(dims[-1], 2 * embed, embed, bias=(True, False))))


class LitResBlock(nn.Module):
    def __init__(self, width, heads):
        super().__init__()
        import collections
        self.ln_1 = nn.LayerNorm(width)
        self.attn = nn.MultiheadAttention(width, heads)
        self.ln_2 = nn.LayerNorm(width)
        self.mlp = nn.Sequential(collections.OrderedDict(c_fc=nn.Linear(width, 4 * width), gelu=nn.GELU(), c_proj=nn.Linear(4 * width, width)))

    def forward(self, x, attn_mask):
        y = self.ln_1(x)
        x = x + self.attn(y, y, y, need_weights=False, attn_mask=attn_mask)[0]
        return x + self.mlp(self.ln_2(x))


class LitTransformer(nn.Module):
    def __init__(self, width, heads, layers):
        super().__init__()
        self.resblocks = nn.ModuleList([LitResBlock(width, heads) for _ in range(layers)])

    def get_cast_dtype(self):
        return self.resblocks[0].mlp.c_fc.weight.dtype

    def forward(self, x, attn_mask=None):                         # LND
        for r in self.resblocks:
            x = r(x, attn_mask)
        return x


class LitCLIP(nn.Module):
    """open_clip's CLIP with a timm ConvNeXt tower, literally; the members ov_dvis/backbones/clip.py touches."""

    def __init__(self, dims, depths, embed, head, text, context=77, vocab=49408):
        super().__init__()
        width, heads, layers = text
        self.visual = LitVisual(dims, depths, embed, head)
        self.transformer = LitTransformer(width, heads, layers)
        self.token_embedding = nn.Embedding(vocab, width)
        self.positional_embedding = nn.Parameter(torch.empty(context, width))
        self.ln_final = nn.LayerNorm(width)
        self.text_projection = nn.Parameter(torch.empty(width, embed))
        self.logit_scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))
        self.register_buffer("attn_mask", torch.full((context, context), float("-inf")).triu_(1), persistent=False)

    # clip.py:117-127, :147-152, :88-100 on this model
    def extract_features(self, x):
        out = {}
        x = self.visual.trunk.stem(x)
        out["stem"] = x.contiguous()
        for i in range(4):
            x = self.visual.trunk.stages[i](x)
            out[f"res{i + 2}"] = x.contiguous()
        out["clip_vis_dense"] = self.visual.trunk.norm_pre(x).contiguous()
        return out

    def visual_prediction_forward(self, x):
        batch, num_query, channel = x.shape
        x = self.visual.head(self.visual.trunk.head(x.reshape(batch * num_query, channel, 1, 1)))
        return x.view(batch, num_query, x.shape[-1])

    def encode_text(self, text):
        x = self.token_embedding(text) + self.positional_embedding
        x = self.transformer(x.permute(1, 0, 2), attn_mask=self.attn_mask).permute(1, 0, 2)
        x = self.ln_final(x)
        return x[torch.arange(x.shape[0]), text.argmax(dim=-1)] @ self.text_projection


TOY = dict(dims=(8, 16, 32, 64), depths=(1, 1, 2, 1), embed=24, text=(32, 2, 2), context=9, vocab=50)


def toy_model_cfg(head):
    return dict(TOY, head=head)


def randomize_(model, seed=0):
    """Every parameter off its initial value, seeded: weights ~ N(0, fan-in scaled), norm weights around 1, biases and the layer scale
    `gamma` of order 0.1 - 1 (at timm's 1e-6 initial value a block would be an identity to fp32)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            leaf = name.rsplit(".", 1)[-1]
            if name.endswith("logit_scale"):
                p.fill_(math.log(30.0))
            elif leaf == "gamma":
                p.copy_(0.5 + 0.5 * torch.rand(p.shape, generator=g))
            elif p.dim() == 1 and leaf == "weight":
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1 or leaf in ("bias", "in_proj_bias"):
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
            elif leaf == "positional_embedding":
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            else:
                fan_in = p[0].numel() if p.dim() > 1 else p.numel()
                p.copy_(torch.randn(p.shape, generator=g) * fan_in ** -0.5)
    return model


def toy_frames(seed=0, B=2, H=37, W=53, pad_to=64):
    """(B, 3, H, W) normalised-image-like frames, zero-padded to pad_to x pad_to (None: as they are)."""
    x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed))
    return x if pad_to is None else F.pad(x, (0, pad_to - W, 0, pad_to - H))


def toy_tokens(seed=0, n=5, context=9, vocab=50):
    """Random token ids whose arg-max (the end-of-text position clip.py reads) falls on a different position in every row."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(1, vocab - 1, (n, context), generator=g)
    for i in range(n):
        t[i, (2 * i + 1) % context] = vocab - 1
    return t


def toy_tokenizer(texts, context=TOY["context"], vocab=TOY["vocab"]):
    """Deterministic: word -> 1 + (sum of its bytes * 31 + its length) % (vocab - 2); the end-of-text id vocab - 1 follows the words."""
    if isinstance(texts, str):
        texts = [texts]
    out = torch.zeros(len(texts), context, dtype=torch.long)
    for i, t in enumerate(texts):
        ids = [1 + (sum(w.encode()) * 31 + len(w)) % (vocab - 2) for w in t.replace(".", " ").replace("{", " ").replace("}", " ").split()]
        ids = ids[-(context - 1):] + [vocab - 1]
        out[i, :len(ids)] = torch.tensor(ids)
    return out
