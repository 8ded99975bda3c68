"""Masked-attention transformer decoder — host side of SURVEY.md §8 rows a6, a7, a8.

Mirrors (constructor arguments, attribute names, ``state_dict`` keys):
  SelfAttentionLayer / CrossAttentionLayer / FFNLayer / MLP
        mask2former_video/modeling/transformer_decoder/video_mask2former_transformer_decoder.py:18-206
  VideoMultiScaleMaskedTransformerDecoder_dvisPlus     dvis_Plus/video_mask2former_transformer_decoder.py:174-374
  VideoMultiScaleMaskedTransformerDecoder_minvis/_dvis ibid. :11-171 (same layers, no re-id head)
  MultiScaleMaskedTransformerDecoder (image, BASELINE config #1)
        mask2former/modeling/transformer_decoder/mask2former_transformer_decoder.py:207-461
  MaskPooling / get_classification_logits / VideoMultiScaleMaskedTransformerDecoder_dvis_OV / _minvis_OV (open vocabulary: the
        FC-CLIP class head on Fn.mask_pool and Fn.text_class_logits; inference only)
        ov_dvis/video_mask2former_transformer_decoder_ov.py:17-377

Inference-only re-organisation for MI355X (same numbers as the reference's eval path):
  * frames are the batch; the K / V projections of ALL layers that read a feature level are ONE GEMM per level
    (the memory does not depend on the queries), done before the layer loop;
  * attention = hand-written fp32-MFMA kernel on strided slices of those GEMM outputs (no (B*8, Q, HW)
    probability tensor, no per-head mask copies);
  * forward_prediction_heads = one fused kernel per layer (contraction + bilinear down-sizing + threshold);
    full-resolution logits are only produced on request, class logits only for the last layer
    (the reference computes and discards the others in eval);
  * the "row blocked everywhere" reset needs no host sync (allowed_count travels with the mask).

Under ``.train()`` all four classes run ``_train_layers`` instead: the reference's training forward (L + 1 predictions,
``aux_outputs``, the (b t) -> (b, t) split by ``num_frames``) as torch ops under autograd around ``Fn.masked_attention``
(cross-attention; backward csrc/masked_attention_backward.hip), ``Fn.attention`` (self-attention) and ``Fn.mask_logits``.
The training maths of a layer is its class's ``train_forward`` — the one spelling the decoders, the tracker and the refiner call.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn

from . import derived, functions as Fn
from .pixel_decoder import ConvNorm, PositionEmbeddingSine, c2_xavier_fill
from .d2 import configurable
from .registry import TRANSFORMER_DECODER_REGISTRY


def _xavier_(module):
    for p in module.parameters():
        if p.dim() > 1:
            nn.init.xavier_uniform_(p)


class SelfAttentionLayer(nn.Module):
    own_gemm = None      # None: the frame-invariant own GEMM of Fn.linear (segmenter); the tracker / refiner set True on their layers

    def __init__(self, d_model, nhead, dropout=0.0, activation="relu", normalize_before=False):
        super().__init__()
        if normalize_before:
            raise NotImplementedError("PRE_NORM=True is not used by the DVIS++ configs")
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)   # parameter container
        self.norm = nn.LayerNorm(d_model)
        self.nhead = nhead
        _xavier_(self)

    def forward(self, tgt, tgt_mask=None, tgt_key_padding_mask=None, query_pos=None):
        assert tgt_mask is None and tgt_key_padding_mask is None
        C = tgt.shape[-1]
        W, b = self.self_attn.in_proj_weight, self.self_attn.in_proj_bias
        own = self.own_gemm
        if query_pos is None:
            qkv = Fn.linear(tgt, W, b, own=own)
            q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        else:
            qk = Fn.linear(tgt + query_pos, W[:2 * C], b[:2 * C], own=own)
            q, k = qk[..., :C], qk[..., C:]
            v = Fn.linear(tgt, W[2 * C:], b[2 * C:], own=own)
        att = Fn.attention(q, k, v, self.nhead)
        op = self.self_attn.out_proj
        return Fn.add_layer_norm(Fn.linear(att, op.weight, op.bias, own=own), tgt, self.norm)

    def train_forward(self, tgt, attend, query_pos=None):
        """``forward`` as torch ops on the live parameters (fused / split projection as there); attend(q, k, v) -> attention."""
        C = tgt.shape[-1]
        W, b = self.self_attn.in_proj_weight, self.self_attn.in_proj_bias
        if query_pos is None:
            qkv = F.linear(tgt, W, b)
            q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        else:
            qk = F.linear(tgt + query_pos, W[:2 * C], b[:2 * C])
            q, k = qk[..., :C], qk[..., C:]
            v = F.linear(tgt, W[2 * C:], b[2 * C:])
        op = self.self_attn.out_proj
        return self.norm(tgt + F.linear(attend(q, k, v), op.weight, op.bias))


class CrossAttentionLayer(nn.Module):
    own_gemm = None

    def __init__(self, d_model, nhead, dropout=0.0, activation="relu", normalize_before=False):
        super().__init__()
        if normalize_before:
            raise NotImplementedError("PRE_NORM=True is not used by the DVIS++ configs")
        self.multihead_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.norm = nn.LayerNorm(d_model)
        self.nhead = nhead
        _xavier_(self)

    def project_q(self, x):
        C = x.shape[-1]
        return Fn.linear(x, self.multihead_attn.in_proj_weight[:C], self.multihead_attn.in_proj_bias[:C],
                         own=self.own_gemm)

    def kv_weights(self):
        C = self.multihead_attn.embed_dim
        W, b = self.multihead_attn.in_proj_weight, self.multihead_attn.in_proj_bias
        return W[C:2 * C], b[C:2 * C], W[2 * C:], b[2 * C:]

    def attend(self, tgt, q_in, k_proj, v_proj, mask=None, allowed=None, identity=None):
        """k_proj / v_proj are already projected (Lk, B, C) views."""
        att = Fn.attention(self.project_q(q_in), k_proj, v_proj, self.nhead, mask, allowed)
        res = tgt if identity is None else identity
        op = self.multihead_attn.out_proj
        return Fn.add_layer_norm(Fn.linear(att, op.weight, op.bias, own=self.own_gemm), res, self.norm)

    def forward(self, tgt, memory, memory_mask=None, memory_key_padding_mask=None, pos=None, query_pos=None):
        assert memory_key_padding_mask is None
        Wk, bk, Wv, bv = self.kv_weights()
        k = Fn.linear(memory if pos is None else memory + pos, Wk, bk, own=self.own_gemm)
        v = Fn.linear(memory, Wv, bv, own=self.own_gemm)
        q_in = tgt if query_pos is None else tgt + query_pos
        return self.attend(tgt, q_in, k, v, memory_mask)

    def train_forward(self, tgt, q_in, k_in, v_in, attend):
        """Residual `tgt`, un-projected q / k / v inputs: torch ops on the live parameters; attend(q, k, v) -> attention."""
        C = tgt.shape[-1]
        W, b = self.multihead_attn.in_proj_weight, self.multihead_attn.in_proj_bias
        att = attend(F.linear(q_in, W[:C], b[:C]), F.linear(k_in, W[C:2 * C], b[C:2 * C]), F.linear(v_in, W[2 * C:], b[2 * C:]))
        op = self.multihead_attn.out_proj
        return self.norm(tgt + F.linear(att, op.weight, op.bias))


class FFNLayer(nn.Module):
    own_gemm = None

    def __init__(self, d_model, dim_feedforward=2048, dropout=0.0, activation="relu", normalize_before=False):
        super().__init__()
        if normalize_before:
            raise NotImplementedError("PRE_NORM=True is not used by the DVIS++ configs")
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm = nn.LayerNorm(d_model)
        _xavier_(self)

    def forward(self, tgt):
        h = Fn.linear_relu(tgt, self.linear1, own=self.own_gemm)
        return Fn.add_layer_norm(Fn.linear(h, self.linear2.weight, self.linear2.bias, own=self.own_gemm), tgt, self.norm)

    def train_forward(self, tgt):
        h = torch.relu(F.linear(tgt, self.linear1.weight, self.linear1.bias))
        return self.norm(tgt + F.linear(h, self.linear2.weight, self.linear2.bias))


class MLP(nn.Module):
    own_gemm = None

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = Fn.linear(x, layer.weight, layer.bias, relu=i < self.num_layers - 1, own=self.own_gemm)
        return x

    def train_forward(self, x):
        for i, layer in enumerate(self.layers):
            x = F.linear(x, layer.weight, layer.bias)
            x = torch.relu(x) if i < self.num_layers - 1 else x
        return x


def layer_predictions(logits, masks):
    """Per-layer class logits and masks (lists, or tensors with a leading layer dimension): the last is the prediction."""
    return {"pred_logits": logits[-1], "pred_masks": masks[-1],
            "aux_outputs": [{"pred_logits": a, "pred_masks": m} for a, m in zip(logits[:-1], masks[:-1])]}


def layer_mask_logits(mask_embed, mask_features, mask_logits):
    """mask_embed (l, b, t, q, cm), mask_features (b, t, cm, h, w) as a constant, b = 1 -> the (l, b, q, t, h, w) view of ONE
    `mask_logits(rows, features)` call (Fn.mask_logits, or Fn.projected_mask_logits with its weights): a frame's rows are l x q."""
    L, _, T, Q, cm = mask_embed.shape
    h, w = mask_features.shape[-2:]
    rows = mask_embed[:, 0].permute(1, 0, 2, 3).reshape(T, L * Q, cm)
    logits = mask_logits(rows, mask_features[0].detach().contiguous())          # (t, l q, h, w)
    return logits.view(T, L, Q, h, w).permute(1, 2, 0, 3, 4).unsqueeze(1)


class _MaskedDecoderBase(nn.Module):
    """Shared body of the image / video masked-attention decoders."""

    _version = 2

    @configurable
    def __init__(self, in_channels, mask_classification=True, *, num_classes, hidden_dim, num_queries, nheads,
                 dim_feedforward, dec_layers, pre_norm, mask_dim, enforce_input_project):
        super().__init__()
        assert mask_classification, "Only support mask classification model"
        self.mask_classification = mask_classification
        self.pe_layer = PositionEmbeddingSine(hidden_dim // 2, normalize=True)
        self.num_heads, self.num_layers = nheads, dec_layers
        self.transformer_self_attention_layers = nn.ModuleList()
        self.transformer_cross_attention_layers = nn.ModuleList()
        self.transformer_ffn_layers = nn.ModuleList()
        for _ in range(self.num_layers):
            self.transformer_self_attention_layers.append(
                SelfAttentionLayer(d_model=hidden_dim, nhead=nheads, dropout=0.0, normalize_before=pre_norm))
            self.transformer_cross_attention_layers.append(
                CrossAttentionLayer(d_model=hidden_dim, nhead=nheads, dropout=0.0, normalize_before=pre_norm))
            self.transformer_ffn_layers.append(
                FFNLayer(d_model=hidden_dim, dim_feedforward=dim_feedforward, dropout=0.0, normalize_before=pre_norm))
        self.decoder_norm = nn.LayerNorm(hidden_dim)
        self.num_queries = num_queries
        self.query_feat = nn.Embedding(num_queries, hidden_dim)
        self.query_embed = nn.Embedding(num_queries, hidden_dim)
        self.num_feature_levels = 3
        self.level_embed = nn.Embedding(self.num_feature_levels, hidden_dim)
        self.input_proj = nn.ModuleList()
        for _ in range(self.num_feature_levels):
            if in_channels != hidden_dim or enforce_input_project:
                self.input_proj.append(ConvNorm(in_channels, hidden_dim, kernel_size=1))
                c2_xavier_fill(self.input_proj[-1])
            else:
                self.input_proj.append(nn.Sequential())
        self.class_embed = nn.Linear(hidden_dim, num_classes + 1)
        self.mask_embed = MLP(hidden_dim, hidden_dim, mask_dim, 3)
        self._kv_cache = derived.Derived()
        self.debug_masks = None      # tests: a list here receives every layer's effective attention mask (N, Q, hw) bool

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        # version shim of the reference (video_mask2former_transformer_decoder.py:213-234): static_query -> query_feat
        version = local_metadata.get("version", None)
        if version is None or version < 2:
            for k in list(state_dict.keys()):
                if k.startswith(prefix) and "static_query" in k:
                    state_dict[k.replace("static_query", "query_feat")] = state_dict.pop(k)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    @staticmethod
    def _base_from_config(cfg, in_channels, mask_classification):
        mf = cfg.MODEL.MASK_FORMER
        assert mf.DEC_LAYERS >= 1
        return dict(in_channels=in_channels, mask_classification=mask_classification,
                    num_classes=cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES, hidden_dim=mf.HIDDEN_DIM,
                    num_queries=mf.NUM_OBJECT_QUERIES, nheads=mf.NHEADS, dim_feedforward=mf.DIM_FEEDFORWARD,
                    dec_layers=mf.DEC_LAYERS - 1, pre_norm=mf.PRE_NORM, enforce_input_project=mf.ENFORCE_INPUT_PROJ,
                    mask_dim=cfg.MODEL.SEM_SEG_HEAD.MASK_DIM)

    # ---- K / V projection weights of all layers reading level l, concatenated once
    def _level_kv_weights(self):
        def make():
            per_level = []
            for lvl in range(self.num_feature_levels):
                idx = [i for i in range(self.num_layers) if i % self.num_feature_levels == lvl]
                ws = [self.transformer_cross_attention_layers[i].kv_weights() for i in idx]
                if not ws:
                    per_level.append(None)
                    continue
                Wv, bv = torch.cat([w[2] for w in ws], 0).detach(), torch.cat([w[3] for w in ws], 0).detach()
                # V = (tok + level_embed) Wv^T + bv = tok Wv^T + (bv + Wv level_embed): the folded bias, made once per weights
                bv_le = (bv.double() + Wv.double() @ self.level_embed.weight[lvl].detach().double()).float()
                per_level.append((tuple(idx), torch.cat([w[0] for w in ws], 0).detach(), torch.cat([w[1] for w in ws], 0).detach(),
                                  Wv, bv, bv_le))
            return tuple(per_level)
        return self._kv_cache.get([t for l in self.transformer_cross_attention_layers
                                   for t in (l.multihead_attn.in_proj_weight, l.multihead_attn.in_proj_bias)]
                                  + [self.level_embed.weight], make)

    @staticmethod
    def _f32_inputs(x, mask_features):
        """Maps handed over by a half-precision region outside the island (a foreign backbone / pixel decoder under autocast)."""
        if any(m.dtype != torch.float32 for m in x):
            tokens = getattr(x, "tokens", None)
            x = type(x)(Fn.f32(m) for m in x)
            if tokens is not None:
                x.tokens = [Fn.f32(t) for t in tokens]
        return x, Fn.f32(mask_features)

    def _run_layers(self, x, mask_features):
        """x: 3 feature maps (N, C, h_l, w_l), low-res first; mask_features (N, Cm, H, W).
        Returns the un-normed residual stream (Q, N, C) after the last layer."""
        C = self.decoder_norm.weight.shape[0]
        N = x[0].shape[0]
        size_list, kproj, vproj = [], {}, {}
        kvw = self._level_kv_weights()
        tokens = getattr(x, "tokens", None)
        with Fn.x3_stage("decoder_kv"):
            for lvl in range(self.num_feature_levels):
                h, w = x[lvl].shape[-2:]
                size_list.append((h, w))
                if kvw[lvl] is None:
                    continue
                idx, Wk, bk, Wv, bv, bv_le = kvw[lvl]
                le = self.level_embed.weight[lvl]
                ident = isinstance(self.input_proj[lvl], nn.Sequential) and len(self.input_proj[lvl]) == 0
                if tokens is not None and ident and not torch.is_grad_enabled():
                    # token-major fast path: K = (tok + level_embed + pos) Wk^T + bk with ONE add pass on the (N, hw, C) tokens;
                    # V = (tok + level_embed) Wv^T + bv = tok Wv^T + (bv + Wv level_embed): no pass at all
                    tok = tokens[lvl]                                                               # (N, hw, C)
                    pos_t = self.pe_layer.compute(h, w, tok.device).flatten(2).transpose(1, 2)      # (1, hw, C)
                    if Fn.x3_on() and Fn.x3_ok(tok, Wk.shape[0], Wk.shape[1], add=True):
                        # every pixel's keys / values for all layers of the level: split-f16 matrix-core GEMM (csrc/gemm_x3.hip)
                        # a level's rows of the encoder memory are read where they lie (dvis_x3_linear_rows); where that entry
                        # does not serve the view, ONE compaction serves both projections
                        if not Fn.x3_rows_in_place(tok, Wk.shape[0]):
                            tok = tok.contiguous()
                        kall = Fn.x3_linear(tok, Wk, bk, xadd=pos_t + le).transpose(0, 1)   # (the (N, hw, C) sum is never written)
                        vall = Fn.x3_linear(tok, Wv, bv_le).transpose(0, 1)
                    else:
                        kall = Fn.linear(tok + (pos_t + le), Wk, bk, tall=True).transpose(0, 1)                # (hw, N, n_l * C) view
                        vall = Fn.linear(tok, Wv, bv_le, tall=True).transpose(0, 1)
                else:
                    src = (self.input_proj[lvl](x[lvl]).flatten(2) + le[None, :, None]).permute(2, 0, 1)
                    pos = self.pe_layer.compute(h, w, x[lvl].device).flatten(2).permute(2, 0, 1)   # (hw, 1, C)
                    kall = Fn.linear(src + pos, Wk, bk, tall=True)                                          # (hw, N, n_l * C)
                    vall = Fn.linear(src, Wv, bv, tall=True)
                for n, i in enumerate(idx):
                    kproj[i], vproj[i] = kall[..., n * C:(n + 1) * C], vall[..., n * C:(n + 1) * C]
        query_embed = self.query_embed.weight.unsqueeze(1)                                      # (Q, 1, C) broadcasts
        output = self.query_feat.weight.unsqueeze(1).repeat(1, N, 1)
        # the attention masks' feature pyramid: the four centre pixels of every 8 x 8 / 4 x 4 / 2 x 2 block of mask_features
        # averaged ONCE (one read of the map) — every layer then contracts its level's small map instead of the stride-4 one
        pyramid = Fn.center_pool3(mask_features)
        if pyramid is not None and [tuple(p.shape[-2:]) for p in pyramid] != [tuple(sz) for sz in size_list[:3]]:
            pyramid = None                                                                      # (levels that are not 1/8, 1/4, 1/2)
        for i in range(self.num_layers):
            lvl = i % self.num_feature_levels
            emb = self.mask_embed(self.decoder_norm(output).transpose(0, 1))                    # (N, Q, Cm)
            if pyramid is not None:
                mask, allowed = Fn.attn_mask_pooled(emb.contiguous(), pyramid[lvl])
            else:
                mask, allowed = Fn.attn_mask(emb.contiguous(), mask_features, size_list[lvl])
            if self.debug_masks is not None:     # rows blocked everywhere attend everywhere (…decoder.py:297)
                self.debug_masks.append(mask.bool() & (allowed > 0)[..., None])
            layer = self.transformer_cross_attention_layers[i]
            output = layer.attend(output, output + query_embed, kproj[i], vproj[i], mask, allowed)
            output = self.transformer_self_attention_layers[i](output, query_pos=query_embed)
            output = self.transformer_ffn_layers[i](output)
        return output

    def _final_heads(self, output, mask_features, need_masks):
        dec = self.decoder_norm(output).transpose(0, 1)                                         # (N, Q, C)
        logits = Fn.linear(dec, self.class_embed.weight, self.class_embed.bias)
        masks = Fn.mask_logits(self.mask_embed(dec).contiguous(), mask_features) if need_masks else None
        return dec, logits, masks

    # ---- training (video_mask2former_transformer_decoder.py:258-379): torch ops under autograd around the attention kernels --------

    def _train_layers(self, x, mask_features):
        """The training forward of the layers and of the heads on the learnable queries and after every layer.
        x: 3 feature maps (N, C, h_l, w_l), low-res first; mask_features (N, Cm, H, W).  Returns (output (Q, N, C) un-normed after
        the last layer, its decoder_norm as (N, Q, C), class logits [L + 1 x (N, Q, K + 1)], mask logits [L + 1 x (N, Q, H, W)]).

        Nothing weight-derived is cached: every layer's K / V projection is an F.linear on the live parameters, so the gradient
        reaches them, input_proj, level_embed and the input maps.  Cross-attention is Fn.masked_attention (forward kernel,
        csrc/masked_attention_backward.hip), self-attention Fn.attention (<= 256 keys: csrc/attention_backward.hip); CPU tensors
        take the torch formulations of both.  A layer's attention mask comes from Fn.attn_mask on the DETACHED embedding (the
        reference detaches at :377).  The mask logits of all L + 1 predictions are ONE Fn.mask_logits call with (L + 1) Q rows per
        frame while mask_features needs no gradient, one call per prediction when it does (that gradient contracts over at most
        256 rows, Fn._mask_logits_grad_features).  No graph capture here."""
        N = x[0].shape[0]
        nh, L = self.num_heads, self.num_layers
        size_list, src, pos = [], [], []
        for lvl in range(self.num_feature_levels):
            h, w = x[lvl].shape[-2:]
            size_list.append((h, w))
            proj = self.input_proj[lvl]
            m = F.conv2d(x[lvl], proj.weight, proj.bias) if isinstance(proj, nn.Conv2d) else proj(x[lvl])
            src.append((m.flatten(2) + self.level_embed.weight[lvl][None, :, None]).permute(2, 0, 1))       # (hw, N, C)
            pos.append(self.pe_layer.compute(h, w, x[lvl].device).to(m.dtype).flatten(2).permute(2, 0, 1))   # (hw, 1, C)
        query_embed = self.query_embed.weight.unsqueeze(1)                                      # (Q, 1, C) broadcasts
        output = self.query_feat.weight.unsqueeze(1).repeat(1, N, 1)
        feats = mask_features.detach()
        logits, embs = [], []

        def heads(output):
            dec = self.decoder_norm(output).transpose(0, 1)                                     # (N, Q, C)
            logits.append(F.linear(dec, self.class_embed.weight, self.class_embed.bias))
            embs.append(self.mask_embed.train_forward(dec))
            return dec

        dec = heads(output)
        for i in range(L):
            lvl = i % self.num_feature_levels
            with torch.no_grad():
                mask, allowed = Fn.attn_mask(embs[-1].detach().contiguous(), feats, size_list[lvl])
            if self.debug_masks is not None:     # rows blocked everywhere attend everywhere (…decoder.py:296)
                self.debug_masks.append(mask.bool() & (allowed > 0)[..., None])
            output = self.transformer_cross_attention_layers[i].train_forward(
                output, output + query_embed, src[lvl] + pos[lvl], src[lvl],
                lambda q, k, v: Fn.masked_attention(q, k, v, nh, mask, allowed))
            output = self.transformer_self_attention_layers[i].train_forward(
                output, lambda q, k, v: Fn.attention(q, k, v, nh), query_pos=query_embed)
            output = self.transformer_ffn_layers[i].train_forward(output)
            dec = heads(output)
        Q = output.shape[0]
        if mask_features.requires_grad and torch.is_grad_enabled():
            masks = [Fn.mask_logits(e.contiguous(), mask_features) for e in embs]
        else:
            masks = list(Fn.mask_logits(torch.cat(embs, dim=1), feats).split(Q, dim=1))
        return output, dec, logits, masks

    def _train_inputs(self, x, mask_features):
        """The maps in the parameters' dtype: fp32; a module moved to double (tests: the fp64 yardstick) stays there."""
        assert len(x) == self.num_feature_levels
        dt = self.decoder_norm.weight.dtype
        return [m.to(dt) for m in x], mask_features.to(dt).contiguous()

    @staticmethod
    def _train_video_outputs(b, t, logits, masks):
        """'(b t) q c -> b t q c' and '(b t) q h w -> b q t h w' of all L + 1 predictions; the first L are the aux_outputs."""
        return layer_predictions([z.unflatten(0, (b, t)) for z in logits],
                                 [z.unflatten(0, (b, t)).transpose(1, 2) for z in masks])

    @staticmethod
    def _train_bctq(z, b, t):
        return z.unflatten(0, (b, t)).permute(0, 3, 1, 2)                                        # ((b t),Q,C) -> (b,C,t,Q)

    def _train_clips(self, N):
        """(b, t) of the (b t) frames of a training batch (…decoder.py:327-329)."""
        t = self.num_frames
        if t < 1 or N % t:
            raise ValueError(f"{type(self).__name__}: a training batch holds (b t) frames with t = num_frames = {t}; got {N} frames")
        return N // t, t


@TRANSFORMER_DECODER_REGISTRY.register()
class MultiScaleMaskedTransformerDecoder(_MaskedDecoderBase):
    """Image Mask2Former decoder (BASELINE config #1).  aux_outputs: the first L of the L + 1 predictions under .train(), [] in eval."""

    @classmethod
    def from_config(cls, cfg, in_channels, mask_classification):
        return cls._base_from_config(cfg, in_channels, mask_classification)

    @Fn.fp32_island
    def forward(self, x, mask_features, mask=None):
        assert len(x) == self.num_feature_levels
        if self.training:
            x, mask_features = self._train_inputs(x, mask_features)
            _, _, logits, masks = self._train_layers(x, mask_features)
            return layer_predictions(logits, masks)
        x, mask_features = self._f32_inputs(x, mask_features)
        output = self._run_layers(x, mask_features)
        _, logits, masks = self._final_heads(output, mask_features, True)
        return {"pred_logits": logits, "pred_masks": masks, "aux_outputs": []}


@TRANSFORMER_DECODER_REGISTRY.register()
class VideoMultiScaleMaskedTransformerDecoder_dvisPlus(_MaskedDecoderBase):
    @configurable
    def __init__(self, in_channels, mask_classification=True, *, num_classes, hidden_dim, num_queries, nheads,
                 dim_feedforward, dec_layers, pre_norm, mask_dim, enforce_input_project, num_frames,
                 num_reid_head_layers, reid_hidden_dim):
        super().__init__(in_channels, mask_classification, num_classes=num_classes, hidden_dim=hidden_dim,
                         num_queries=num_queries, nheads=nheads, dim_feedforward=dim_feedforward,
                         dec_layers=dec_layers, pre_norm=pre_norm, mask_dim=mask_dim,
                         enforce_input_project=enforce_input_project)
        self.num_frames = num_frames
        if num_reid_head_layers > 0:
            self.reid_embed = MLP(hidden_dim, reid_hidden_dim, hidden_dim, num_reid_head_layers)
            for layer in self.reid_embed.layers:
                c2_xavier_fill(layer)
        else:
            self.reid_embed = nn.Identity()
        self.compute_pred_masks = True     # the offline / online meta-architectures switch this off (unused there)

    @classmethod
    def from_config(cls, cfg, in_channels, mask_classification):
        ret = cls._base_from_config(cfg, in_channels, mask_classification)
        ret.update(num_frames=cfg.INPUT.SAMPLING_FRAME_NUM, reid_hidden_dim=cfg.MODEL.MASK_FORMER.REID_HIDDEN_DIM,
                   num_reid_head_layers=cfg.MODEL.MASK_FORMER.NUM_REID_HEAD_LAYERS)
        return ret

    @Fn.fp32_island
    def forward(self, x, mask_features, mask=None):
        """Eval semantics of the reference (bs = 1: all frames form one clip).  Shapes as in the reference:
        pred_logits (1,T,Q,K+1), pred_masks (1,Q,T,H,W) or None, pred_embds / pred_embds_without_norm (1,2C,T,Q),
        pred_reid_embed (1,C,T,Q), mask_features (T,Cm,H,W)."""
        assert len(x) == self.num_feature_levels
        if self.training:
            return self._forward_train(x, mask_features)
        x, mask_features = self._f32_inputs(x, mask_features)
        output = self._run_layers(x, mask_features)
        dec, logits, masks = self._final_heads(output, mask_features, self.compute_pred_masks)
        reid = self.reid_embed(dec)                                                              # (T, Q, C)
        to_bctq = lambda z: z.permute(2, 0, 1).unsqueeze(0)                                      # (T,Q,C) -> (1,C,T,Q)
        reid_b = to_bctq(reid)
        return {
            "pred_logits": logits.unsqueeze(0),
            "pred_masks": None if masks is None else masks.permute(1, 0, 2, 3).unsqueeze(0),
            "aux_outputs": [],
            "pred_embds": torch.cat([to_bctq(dec), reid_b], dim=1),
            "pred_embds_without_norm": torch.cat([output.permute(2, 1, 0).unsqueeze(0), reid_b], dim=1),
            "pred_reid_embed": reid_b,
            "mask_features": mask_features,
        }


    def _forward_train(self, x, mask_features):
        """Training semantics of the reference (…decoder.py:326-354): the (b t) frames are b clips of num_frames; pred_logits
        (b,t,Q,K+1), pred_masks (b,Q,t,H,W) — always computed, compute_pred_masks is an inference switch —, aux_outputs for the
        learnable queries and the first L - 1 layers, embeddings (b,·,t,Q) composed as in eval."""
        x, mask_features = self._train_inputs(x, mask_features)
        b, t = self._train_clips(x[0].shape[0])
        output, dec, logits, masks = self._train_layers(x, mask_features)
        out = self._train_video_outputs(b, t, logits, masks)
        reid = self.reid_embed
        reid_b = self._train_bctq(reid.train_forward(dec) if isinstance(reid, MLP) else reid(dec), b, t)   # (nn.Identity: no head)
        out.update(pred_embds=torch.cat([self._train_bctq(dec, b, t), reid_b], dim=1),
                   pred_embds_without_norm=torch.cat([self._train_bctq(output.transpose(0, 1), b, t), reid_b], dim=1),
                   pred_reid_embed=reid_b, mask_features=mask_features)
        return out


@TRANSFORMER_DECODER_REGISTRY.register()
class VideoMultiScaleMaskedTransformerDecoder_dvis(_MaskedDecoderBase):
    """DVIS (v1) per-frame decoder: single-branch embeddings, no re-id head (dvis_Plus/…decoder.py:11-145)."""

    @configurable
    def __init__(self, in_channels, mask_classification=True, *, num_classes, hidden_dim, num_queries, nheads,
                 dim_feedforward, dec_layers, pre_norm, mask_dim, enforce_input_project, num_frames):
        super().__init__(in_channels, mask_classification, num_classes=num_classes, hidden_dim=hidden_dim,
                         num_queries=num_queries, nheads=nheads, dim_feedforward=dim_feedforward,
                         dec_layers=dec_layers, pre_norm=pre_norm, mask_dim=mask_dim,
                         enforce_input_project=enforce_input_project)
        self.num_frames = num_frames

    @classmethod
    def from_config(cls, cfg, in_channels, mask_classification):
        ret = cls._base_from_config(cfg, in_channels, mask_classification)
        ret.update(num_frames=cfg.INPUT.SAMPLING_FRAME_NUM)
        return ret

    @Fn.fp32_island
    def forward(self, x, mask_features, mask=None):
        if self.training:
            x, mask_features = self._train_inputs(x, mask_features)
            b, t = self._train_clips(x[0].shape[0])
            output, dec, logits, masks = self._train_layers(x, mask_features)
            out = self._train_video_outputs(b, t, logits, masks)
            out.update(pred_embds=self._train_bctq(dec, b, t), pred_embds_without_norm=self._train_bctq(output.transpose(0, 1), b, t),
                       mask_features=mask_features)
            return out
        x, mask_features = self._f32_inputs(x, mask_features)
        output = self._run_layers(x, mask_features)
        dec, logits, masks = self._final_heads(output, mask_features, True)
        return {"pred_logits": logits.unsqueeze(0), "pred_masks": masks.permute(1, 0, 2, 3).unsqueeze(0),
                "aux_outputs": [], "pred_embds": dec.permute(2, 0, 1).unsqueeze(0),
                "pred_embds_without_norm": output.permute(2, 1, 0).unsqueeze(0), "mask_features": mask_features}


@TRANSFORMER_DECODER_REGISTRY.register()
class VideoMultiScaleMaskedTransformerDecoder_minvis(VideoMultiScaleMaskedTransformerDecoder_dvis):
    """MinVIS: the `_dvis` decoder without `mask_features` in its outputs (…decoder.py:164-171)."""

    def forward(self, x, mask_features, mask=None):
        out = super().forward(x, mask_features, mask=mask)
        del out["mask_features"]
        return out


# ---- open-vocabulary (FC-CLIP) heads: ov_dvis/video_mask2former_transformer_decoder_ov.py ---------------------------------------------

def get_classification_logits(x, text_classifier, logit_scale, num_templates=None):
    """…decoder_ov.py:17-36: x (B, *, C), text_classifier (N, C), logit_scale a scalar parameter, num_templates the templates per
    class with the void group last -> (B, *, K + 1).  One GEMM and one epilogue launch (Fn.text_class_logits)."""
    return Fn.text_class_logits(x, text_classifier, logit_scale, num_templates)


class MaskPooling(nn.Module):
    """…decoder_ov.py:39-67: the mean of x (B, C, H, W) under every query's own mask (`logit > 0`) -> (B, Q, C); return_num also
    returns the denominators (B, Q, 1, 1) = pixel count + 1e-8.  Masks of another size are resized first, with torch as in the
    reference.  The binary mask tensor is never written (Fn.mask_pool)."""

    def forward(self, x, mask, return_num=False):
        if not x.shape[-2:] == mask.shape[-2:]:
            mask = F.interpolate(mask, size=x.shape[-2:], mode="bilinear", align_corners=False)
        pooled, denorm = Fn.mask_pool_mean(x, mask.detach())
        return (pooled, denorm) if return_num else pooled


@TRANSFORMER_DECODER_REGISTRY.register()
class VideoMultiScaleMaskedTransformerDecoder_dvis_OV(_MaskedDecoderBase):
    """The per-frame decoder of the open-vocabulary family (…decoder_ov.py:69-366): the layers of `_dvis`, and a class head that
    has no Linear(hidden, K + 1) — a query is classified by the mean of mask_features under its own mask, projected, added to the
    normalised query, taken to CLIP space by a 3-layer MLP and compared with the text classifier's rows.

    Inference only.  Eval returns the last prediction (`aux_outputs` is [], as for the other decoders); under ``.train()`` within
    ``torch.no_grad()`` — how the open-vocabulary tracker and refiner stages run the frozen segmenter — all L + 1 predictions come
    back, the (b t) frames split by num_frames, computed by the SAME layer and head calls as in eval: the last one equals eval's bit
    for bit.  With grad enabled and a trainable parameter the forward raises: mask pooling and the text logits have no backward."""

    @configurable
    def __init__(self, in_channels, mask_classification=True, *, num_classes, hidden_dim, num_queries, nheads,
                 dim_feedforward, dec_layers, pre_norm, mask_dim, enforce_input_project, clip_embedding_dim, num_frames):
        super().__init__(in_channels, mask_classification, num_classes=num_classes, hidden_dim=hidden_dim,
                         num_queries=num_queries, nheads=nheads, dim_feedforward=dim_feedforward,
                         dec_layers=dec_layers, pre_norm=pre_norm, mask_dim=mask_dim,
                         enforce_input_project=enforce_input_project)
        self.num_frames = num_frames
        self.mask_pooling = MaskPooling()
        self._mask_pooling_proj = nn.Sequential(nn.LayerNorm(hidden_dim), nn.Linear(hidden_dim, hidden_dim))
        self.class_embed = MLP(hidden_dim, hidden_dim, clip_embedding_dim, 3)      # (replaces the closed-vocabulary Linear)
        self.logit_scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))
        self.debug_pooled = None     # tests: a list here receives every prediction's (pooled embeddings (N, Q, C), counts (N, Q))

    @classmethod
    def from_config(cls, cfg, in_channels, mask_classification):
        ret = cls._base_from_config(cfg, in_channels, mask_classification)
        ret.update(num_frames=cfg.INPUT.SAMPLING_FRAME_NUM, clip_embedding_dim=cfg.MODEL.FC_CLIP.EMBED_DIM)
        return ret

    def forward_prediction_heads(self, output, mask_features, text_classifier, num_templates):
        """…decoder_ov.py:331-353 without the attention mask (the layers make their own): output (Q, N, C) un-normed ->
        (class logits (N, Q, K + 1), mask logits (N, Q, H, W), decoder_norm(output) as (N, Q, C)).  Mask pooling reads the mask
        logits that were written anyway."""
        dec = self.decoder_norm(output).transpose(0, 1)                                         # (N, Q, C)
        masks = Fn.mask_logits(self.mask_embed(dec).contiguous(), mask_features)
        total, count = Fn.mask_pool(mask_features, masks)
        pooled = total / (count.to(total.dtype) + 1e-8).unsqueeze(-1)                           # MaskPooling's mean
        if self.debug_pooled is not None:
            self.debug_pooled.append((pooled, count))
        norm, proj = self._mask_pooling_proj
        emb = self.class_embed(Fn.linear(norm(pooled), proj.weight, proj.bias) + dec)
        return get_classification_logits(emb, text_classifier, self.logit_scale, num_templates), masks, dec

    @Fn.fp32_island
    def forward(self, x, mask_features, mask=None, text_classifier=None, num_templates=None, clip_size=1):
        """Shapes as in the reference: pred_logits (b, t, Q, K + 1), pred_masks (b, Q, t, H, W), pred_embds /
        pred_embds_without_norm (b, C, t, Q), mask_features ((b t), Cm, H, W); b = 1 in eval."""
        assert len(x) == self.num_feature_levels
        if text_classifier is None or num_templates is None:
            raise ValueError(f"{type(self).__name__}: text_classifier (N, {self.class_embed.layers[-1].out_features}) and "
                             "num_templates are required — an open-vocabulary decoder has no class weights of its own")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError(
                f"{type(self).__name__}: training the open-vocabulary heads is not implemented — mask_pool and text_class_logits have no "
                "backward.  Run the frozen segmenter under torch.no_grad() (in .train() it returns all L + 1 predictions) or freeze its "
                "parameters")
        del mask                                                                                # (the reference disables it too)
        x, mask_features = self._f32_inputs(x, mask_features)
        mask_features = mask_features.contiguous()
        N = x[0].shape[0]
        heads = lambda o: self.forward_prediction_heads(o, mask_features, text_classifier, num_templates)
        if not self.training:
            b, t = 1, N
            output = self._run_layers(x, mask_features)
            preds = [heads(output)]
        else:
            # every layer's residual stream, from the layers of _run_layers themselves: a forward hook on each FFN (a layer's last op)
            b, t = self._train_clips(N)
            streams = [self.query_feat.weight.unsqueeze(1).repeat(1, N, 1)]
            hooks = [ffn.register_forward_hook(lambda m, args, out: streams.append(out)) for ffn in self.transformer_ffn_layers]
            try:
                output = self._run_layers(x, mask_features)
            finally:
                for h in hooks:
                    h.remove()
            assert len(streams) == self.num_layers + 1 and streams[-1] is output
            preds = [heads(o) for o in streams]
        out = self._train_video_outputs(b, t, [p[0] for p in preds], [p[1] for p in preds])
        if not self.training:
            out["aux_outputs"] = []
        out.update(pred_embds=self._train_bctq(preds[-1][2], b, t),
                   pred_embds_without_norm=self._train_bctq(output.transpose(0, 1), b, t), mask_features=mask_features)
        return out


@TRANSFORMER_DECODER_REGISTRY.register()
class VideoMultiScaleMaskedTransformerDecoder_minvis_OV(VideoMultiScaleMaskedTransformerDecoder_dvis_OV):
    """MinVIS open-vocabulary: the `_dvis_OV` decoder without `mask_features` in its outputs (…decoder_ov.py:368-377)."""

    def forward(self, x, mask_features, mask=None, text_classifier=None, num_templates=None, clip_size=1):
        out = super().forward(x, mask_features, mask=mask, text_classifier=text_classifier, num_templates=num_templates,
                              clip_size=clip_size)
        del out["mask_features"]
        return out
