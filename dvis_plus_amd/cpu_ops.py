"""Torch formulations of the four hot ops for CPU TENSORS — BASELINE config #1 read literally ("Mask2Former R50 single 480p
frame, 100 queries, PyTorch CPU MSDeformAttn fallback (plumbing, no GPU)").

The reference ships one such function, ``ms_deform_attn_core_pytorch`` (ops/functions/ms_deform_attn_func.py:52-72), and reaches
it through a bare ``except`` around the CUDA op (ops/modules/ms_deform_attn.py:116-121) — on ANY failure, silently, GPU tensors
included.  Here the dispatch is by device and explicit: a tensor on the CPU takes these functions, a tensor on the GPU takes the
HIP kernel or raises (functions.py: no torch formulation ever runs on a GPU tensor behind the caller's back, a missing / broken
libdvis_hip.so is an error).  Nothing in here is on the measured path, and nothing in here imports ``oracle/`` (test infrastructure).
"""
import torch
import torch.nn.functional as F


def ms_deform_attn_core_pytorch(value, value_spatial_shapes, sampling_locations, attention_weights):
    """Same name, arguments and result as the reference's torch formulation (ms_deform_attn_func.py:52-72):
    value (N, S, M, D), value_spatial_shapes (L, 2) rows (H_l, W_l), sampling_locations (N, Lq, M, L, P, 2) in [0, 1] (x, y),
    attention_weights (N, Lq, M, L, P) -> (N, Lq, M * D).

    out[n, q, m, :] = sum_{l, p} w[n, q, m, l, p] * bilinear(value_l[n, :, m, :], loc[n, q, m, l, p]) with zero padding and
    pixel centres at (i + 0.5) / size: ``F.grid_sample(align_corners=False)`` on 2 loc - 1 per level.  The levels' terms are
    accumulated one after the other (the reference stacks all L * P samples and reduces once: same sum, other association)."""
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = sampling_locations.shape
    shapes = [(int(h), int(w)) for h, w in value_spatial_shapes.tolist()]
    if sum(h * w for h, w in shapes) != S or len(shapes) != L:
        raise RuntimeError("ms_deform_attn_core_pytorch: value rows do not match the spatial shapes")
    grid = 2 * sampling_locations - 1
    out, start = None, 0
    for lvl, (h, w) in enumerate(shapes):
        v = value[:, start:start + h * w].permute(0, 2, 3, 1).reshape(N * M, D, h, w)                  # (N M, D, h, w)
        g = grid[:, :, :, lvl].permute(0, 2, 1, 3, 4).reshape(N * M, Lq, P, 2)                         # (N M, Lq, P, 2)
        s = F.grid_sample(v, g, mode="bilinear", padding_mode="zeros", align_corners=False)           # (N M, D, Lq, P)
        wl = attention_weights[:, :, :, lvl].permute(0, 2, 1, 3).reshape(N * M, 1, Lq, P)
        term = (s * wl).sum(-1)                                                                        # (N M, D, Lq)
        out = term if out is None else out + term
        start += h * w
    return out.view(N, M * D, Lq).transpose(1, 2).contiguous()


def attention(q, k, v, nheads, mask=None, allowed_count=None, out=None):
    """functions.attention for CPU tensors: softmax(q k^T / sqrt(d)) v per head on (L, B, C) tensors; mask (B, Lq, Lk) with
    1 = blocked, rows whose allowed_count is 0 attend everywhere (video_mask2former_transformer_decoder.py:297)."""
    Lq, B, C = q.shape
    Lk, d = k.shape[0], C // nheads
    heads = lambda t, n: t.reshape(n, B, nheads, d).permute(1, 2, 0, 3)                                # (B, H, L, d)
    s = (heads(q, Lq) * (1.0 / d ** 0.5)) @ heads(k, Lk).transpose(-1, -2)
    if mask is not None:
        blocked = mask.bool()
        if allowed_count is not None:
            blocked = blocked & (allowed_count > 0)[..., None]
        s = s.masked_fill(blocked[:, None], float("-inf"))
    o = (torch.softmax(s, -1) @ heads(v, Lk)).permute(2, 0, 1, 3).reshape(Lq, B, C)
    if out is not None:
        out.copy_(o)
        return out
    return o


def mask_logits(mask_embed, mask_features):
    """einsum("bqc,bchw->bqhw") (video_mask2former_transformer_decoder.py:363)."""
    B, Q, C = mask_embed.shape
    H, W = mask_features.shape[-2:]
    return torch.bmm(mask_embed, mask_features.flatten(2)).view(B, Q, H, W)


def attn_mask(mask_embed, mask_features, target_size):
    """functions.attn_mask for CPU tensors (ibid. :363-371): (mask uint8 (B, Q, h w) with 1 = blocked, allowed_count int32 (B, Q))."""
    small = F.interpolate(mask_logits(mask_embed, mask_features), size=(int(target_size[0]), int(target_size[1])), mode="bilinear",
                          align_corners=False)
    blocked = small.sigmoid().flatten(2) < 0.5
    return blocked.to(torch.uint8), (~blocked).sum(-1).to(torch.int32)


# --- video metrics (csrc/video_metrics.hip): the same counts by torch.bincount -------------------------------------------------
def pan_pair_hist(gt, pred, gt_table, num_pred):
    """(T, Ng + 2, Np + 1) int64 pair counts and the number of predictions outside 0..Np (see dvis_pan_pair_hist)."""
    T = gt.shape[0]
    ng, np1 = gt_table.numel(), num_pred + 1
    g, p = gt.reshape(T, -1).long(), pred.reshape(T, -1).long()
    table = gt_table.long()
    pos = torch.searchsorted(table, g).clamp_(max=max(ng - 1, 0))
    found = table[pos] == g if ng else torch.zeros_like(g, dtype=torch.bool)
    row = torch.where(g == 0, 0, torch.where(found, pos + 1, ng + 1))
    ok = (p >= 0) & (p <= num_pred)
    frame = torch.arange(T).view(T, 1).expand_as(g)
    idx = (frame * (ng + 2) + row) * np1 + p
    counts = torch.bincount(idx[ok], minlength=T * (ng + 2) * np1)
    return counts.view(T, ng + 2, np1), int((~ok).sum())


def sem_confusion(gt, pred, num_class):
    """(num_class, num_class) int64 confusion of eval_miou_vspw.py:_generate_matrix and the count of `bad` pixels."""
    g = gt.reshape(-1).long() & 255
    g = (torch.where(g == 0, 255, g) - 1) & 255
    p = pred.reshape(-1).long()
    keep = g < num_class
    b = num_class * g[keep] + p[keep]
    ok = (p[keep] >= 0) & (b < num_class * num_class)
    return torch.bincount(b[ok], minlength=num_class * num_class).view(num_class, num_class), int((~ok).sum())


def video_consistency(gt, pred, ks):
    """(gt_const, both_const), each (len(ks), T) int64: eval_vc_vspw.py:get_common's counts per window start i < T - k."""
    T = gt.shape[0]
    g, p = gt.reshape(T, -1), pred.reshape(T, -1)
    gc = torch.zeros((len(ks), T), dtype=torch.int64)
    bc = torch.zeros((len(ks), T), dtype=torch.int64)
    same_g = g[1:] == g[:-1]                  # frame t + 1 equals frame t
    same_p = p[1:] == p[:-1]
    for j, k in enumerate(ks):
        for i in range(T - k):
            cg = same_g[i:i + k - 1].all(0)
            gc[j, i] = cg.sum()
            bc[j, i] = (cg & same_p[i:i + k - 1].all(0)).sum()
    return gc, bc


# --- VIS scoring (csrc/vis_metrics.hip): COCO RLE and track intersections by plain torch ops -----------------------------------
def _run_index(run_off):
    """(mask of each run, index of each run inside its mask) for runs laid out at run_off (N + 1)."""
    n_runs = run_off[1:] - run_off[:-1]
    mask = torch.repeat_interleave(torch.arange(n_runs.numel()), n_runs)
    return mask, torch.arange(mask.numel()) - run_off[mask]


def rle_encode(masks):
    """(runs int32, run_off (N + 1) int64, area (N) int64) of (N, H, W) masks: COCO runs in column-major order, zeros first."""
    N, H, W = masks.shape
    m = (masks != 0).transpose(1, 2).reshape(N, H * W).to(torch.int8)
    prev = torch.cat((torch.zeros((N, 1), dtype=torch.int8), m[:, :-1]), 1)
    n, pos = torch.nonzero(m != prev, as_tuple=True)            # row-major: by mask, then position
    moff = torch.zeros(N + 1, dtype=torch.int64)
    moff[1:] = torch.bincount(n, minlength=N).cumsum(0)
    run_off = moff + torch.arange(N + 1)
    at = run_off[n] + torch.arange(n.numel()) - moff[n]          # run index that ends at boundary `pos`
    ends = torch.empty(int(run_off[-1]), dtype=torch.int64)
    starts = torch.empty_like(ends)
    ends[at], starts[at + 1] = pos, pos
    ends[run_off[1:] - 1] = H * W
    starts[run_off[:-1]] = 0
    return (ends - starts).to(torch.int32), run_off, m.sum(1, dtype=torch.int64)


def rle_strings(runs, run_off):
    """(chars uint8, str_off (N + 1) int64): cocoapi's rleToString of every mask, concatenated."""
    cnt = runs.long()
    mask, i = _run_index(run_off)
    x = cnt.clone()
    back = i > 2
    x[back] -= cnt[torch.nonzero(back, as_tuple=True)[0] - 2]
    active = torch.ones_like(x, dtype=torch.bool)
    cols = []
    for _ in range(8):                                           # a 33-bit signed delta takes at most 7 groups
        c = x & 0x1f
        x = x >> 5
        more = torch.where((c & 0x10) != 0, x != -1, x != 0)
        cols.append(torch.where(active, torch.where(more, c | 0x20, c) + 48, -1))
        active &= more
    assert not bool(active.any())
    chars = torch.stack(cols, 1)
    valid = chars >= 0
    str_off = torch.zeros(run_off.numel(), dtype=torch.int64)
    str_off[1:] = torch.zeros(run_off.numel() - 1, dtype=torch.int64).index_add_(0, mask, valid.sum(1)).cumsum(0)
    return chars[valid].to(torch.uint8), str_off


def rle_decode(runs, run_off, H, W):
    """(N, H, W) uint8 0 / 1 masks from their runs (each mask's runs must sum to H * W)."""
    N = run_off.numel() - 1
    _, i = _run_index(run_off)
    flat = torch.repeat_interleave((i & 1).to(torch.uint8), runs.long())
    if flat.numel() != N * H * W:
        raise ValueError(f"rle_decode: the runs cover {flat.numel()} pixels, not {N} x {H} x {W}")
    return flat.view(N, W, H).transpose(1, 2).contiguous()


def track_intersections(pred, gt):
    """(P, G) int64: sum over frames of |pred[p, t] & gt[g, t]| for pred (P, T, ...) and gt (G, T, ...) masks."""
    P, G, T = pred.shape[0], gt.shape[0], pred.shape[1]
    out = torch.zeros((P, G), dtype=torch.float64)
    for t in range(T):                                           # float64 sums of 0 / 1 products: exact below 2^53
        a = (pred[:, t] != 0).reshape(P, -1).to(torch.float64)
        b = (gt[:, t] != 0).reshape(G, -1).to(torch.float64)
        out += a @ b.t()
    return out.to(torch.int64)


# --- prediction files (csrc/pred_write.hip): segment stats and painted maps by plain torch ops -------------------------------------
def pan_segment_stats(pan, n):
    """((T, n + 1, 5) int64 area, xmin, ymin, xmax, ymax per frame and id 0..n — all zero where the id has no pixel, bad): the
    ids of the (T, H, W) map outside 0..n are only counted in `bad`."""
    T, H, W = pan.shape
    ids = pan.reshape(T, H * W).long()
    ok = (ids >= 0) & (ids <= n)
    bad = int((~ok).sum())
    key = (torch.arange(T).view(T, 1) * (n + 1) + ids.clamp(0, n))[ok]
    pos = torch.arange(H * W).expand(T, H * W)[ok]
    xs, ys = pos % W, pos // W
    out = torch.zeros((T * (n + 1), 5), dtype=torch.int64)
    out[:, 0] = torch.bincount(key, minlength=T * (n + 1))
    big = torch.full((T * (n + 1),), H * W, dtype=torch.int64)
    out[:, 1] = big.scatter_reduce(0, key, xs, "amin")
    out[:, 2] = big.scatter_reduce(0, key, ys, "amin")
    out[:, 3] = torch.zeros_like(big).scatter_reduce(0, key, xs, "amax")
    out[:, 4] = torch.zeros_like(big).scatter_reduce(0, key, ys, "amax")
    out[out[:, 0] == 0] = 0
    return out.view(T, n + 1, 5), bad


def pan_paint_rgb(pan, lut):
    """(T, H, W, 3) uint8: the colour lut[id] (0x00BBGGRR int32, one per id) of every pixel; ids outside the table are black."""
    ids = pan.long()
    ok = (ids >= 0) & (ids < lut.numel())
    col = torch.where(ok, lut.long()[ids.clamp(0, max(lut.numel() - 1, 0))] if lut.numel() else torch.zeros_like(ids), 0)
    return torch.stack((col & 255, (col >> 8) & 255, (col >> 16) & 255), -1).to(torch.uint8)


def sem_paint(sem, lut):
    """(uint8 lut[sem & 255] of every pixel, bad (256) int64): lut (256) holds the dataset id of each class byte or -1 (no mapping:
    written as 255, counted per class)."""
    c = sem.long() & 255
    d = lut.long()[c]
    return torch.where(d >= 0, d, 255).to(torch.uint8), torch.bincount(c[d < 0].reshape(-1), minlength=256)


# --- test-time frame resize (csrc/frame_resize.hip): Pillow's BILINEAR resample as gathers and integer sums ------------------------
def _resample_axis(x, tab, dim):
    """One pass of Pillow's 8-bit resample along `dim` of the int64 tensor x: tab (n_out, k + 2) = first index, taps, k
    coefficients (zero past the taps, so clamped gathers there add nothing)."""
    n_in = x.shape[dim]
    first, coef = tab[:, 0].long(), tab[:, 2:].long()
    n_out, k = coef.shape
    idx = (first[:, None] + torch.arange(k)[None]).clamp(max=n_in - 1)
    g = x.index_select(dim, idx.reshape(-1))
    g = g.reshape(*x.shape[:dim], n_out, k, *x.shape[dim + 1:])
    c = coef.reshape(n_out, k, *([1] * (x.dim() - dim - 1)))
    acc = (g * c).sum(dim + 1) + (1 << 21)
    return torch.where(acc <= 0, 0, (acc >> 22).clamp(max=255))


def resize_frames_u8(frames, xtab, ytab, reverse=False):
    """(T, 3, h, w) uint8 from (T, H, W, 3) uint8: horizontal pass (xtab) then vertical pass (ytab), each clip8 to uint8 values,
    as Pillow's ImagingResample does; channels reversed if `reverse`."""
    out = []
    for f in frames:
        x = _resample_axis(f.long(), xtab, 1)
        x = _resample_axis(x, ytab, 0)
        out.append((x.flip(-1) if reverse else x).permute(2, 0, 1).to(torch.uint8))
    return torch.stack(out)


# --- set criterion (csrc/criterion.hip): matching cost and point-sampled mask losses on CPU tensors -----------------------------
def point_sample_rows(rows, coords):
    """rows (R, H, W) any real dtype, coords (R, P, 2) normalised (x, y) -> (R, P) fp32: bilinear, zero padding, pixel centres at
    (i + 0.5) / size (grid_sample on 2 c - 1, align_corners=False)."""
    R, P = coords.shape[:2]
    if R == 0 or P == 0:
        return (rows.to(torch.float32).sum() * 0).expand(R, P).clone() if rows.requires_grad \
            else torch.zeros((R, P), dtype=torch.float32, device=coords.device)
    grid = (2.0 * coords.to(torch.float32) - 1.0)[:, :, None, :]
    return F.grid_sample(rows.to(torch.float32)[:, None], grid, mode="bilinear", padding_mode="zeros",
                         align_corners=False)[:, 0, :, 0]


def match_cost_terms(pred, tgt, coords, logits, tgt_ids):
    """pred (Q, T, H, W), tgt (G, T, Ht, Wt), coords (K, 2) shared by every mask and frame, logits (Q, C), tgt_ids (G) ->
    (cost_class, cost_mask, cost_dice), each (Q, G), unweighted."""
    Q, T, H, W = pred.shape
    G, K = tgt.shape[0], coords.shape[0]
    x = point_sample_rows(pred.reshape(Q * T, H, W), coords[None].expand(Q * T, K, 2)).reshape(Q, T * K)
    t = point_sample_rows(tgt.reshape(G * T, *tgt.shape[2:]), coords[None].expand(G * T, K, 2)).reshape(G, T * K)
    cost_class = -logits.to(torch.float32).softmax(-1)[:, tgt_ids.to(torch.int64)]
    cost_mask = (F.softplus(-x) @ t.T + F.softplus(x) @ (1.0 - t).T) / (T * K)
    s = x.sigmoid()
    cost_dice = 1.0 - (2.0 * (s @ t.T) + 1.0) / (s.sum(-1)[:, None] + t.sum(-1)[None, :] + 1.0)
    return cost_class, cost_mask, cost_dice


def point_loss_sums(src, tgt, coords):
    """src, tgt (R, H, W), coords (R, P, 2) -> (R, 3): per row sum_p bce(x, t), sum_p sigmoid(x) t, sum_p sigmoid(x) + sum_p t over
    the sampled values (differentiable in src through torch autograd)."""
    x = point_sample_rows(src, coords)
    t = point_sample_rows(tgt, coords)
    s = x.sigmoid()
    bce = F.softplus(x) - x * t
    return torch.stack((bce.sum(-1), (s * t).sum(-1), s.sum(-1) + t.sum(-1)), dim=-1)


# --- contrastive item losses (csrc/contrastive_items.hip) as batched torch ops ---------------------------------------------------
def contrastive_items(src, anchor, pos_ptr, pos_idx, neg_ptr, neg_idx):
    """functions.contrastive_items as torch ops on src's device and in its dtype (differentiable through torch autograd): src
    (R, C); item i has the anchor row anchor[i], the positive rows pos_idx[pos_ptr[i]:pos_ptr[i + 1]] and the negative rows
    neg_idx[neg_ptr[i]:neg_ptr[i + 1]] (int64 CPU tensors, checked by the caller) -> (reid (n), aux (n)):
    reid = softplus(LSE_j(n_j . a) + LSE_k(-p_k . a)), the separable form of the logsumexp over all (n_j - p_k) . a and one 0 (an
    empty side: 0); aux = (sum_k (cos(p_k, a) - 1)^2 + sum_j cos(n_j, a)^2) / (P + N) with F.normalize's cosine."""
    dev, n = src.device, anchor.numel()
    if n == 0:
        return src.new_zeros(0), src.new_zeros(0)
    a = src[anchor.to(dev)]                                                                     # (n, C)
    ua = F.normalize(a, dim=-1)
    aux_sum, count = src.new_zeros(n), (pos_ptr[-1:] * 0).expand(n).clone()
    lses = []
    for ptr, idx, sign, label in ((neg_ptr, neg_idx, 1.0, 0.0), (pos_ptr, pos_idx, -1.0, 1.0)):
        cnt = ptr[1:] - ptr[:-1]
        count = count + cnt
        m = int(cnt.max())
        if m == 0:
            lses.append(src.new_zeros(n))
            continue
        item = torch.repeat_interleave(torch.arange(n), cnt)
        col = (torch.arange(idx.numel()) - ptr[:-1][item]).to(dev)
        item = item.to(dev)
        x = src[idx.to(dev)]                                                                    # (slots of this side, C)
        dot = (x * a[item]).sum(-1)
        cos = (F.normalize(x, dim=-1) * ua[item]).sum(-1)
        aux_sum = aux_sum.index_add(0, item, (cos - label).square())
        # rows of an item without slots on this side are padded with zeros, not -inf: their LSE is masked out below and its
        # gradient must not be NaN
        pad = torch.where((cnt > 0).to(dev)[:, None], src.new_full((n, m), float("-inf")), src.new_zeros(n, m))
        pad = pad.index_put((item, col), sign * dot)
        lses.append(torch.logsumexp(pad, dim=1))
    both = ((pos_ptr[1:] > pos_ptr[:-1]) & (neg_ptr[1:] > neg_ptr[:-1])).to(dev)
    z = lses[0] + lses[1]
    reid = torch.where(both, torch.logaddexp(z, torch.zeros_like(z)), torch.zeros_like(z))
    aux = aux_sum / count.clamp(min=1).to(device=dev, dtype=src.dtype)
    return reid, aux


# --- shifted-window attention of the Swin backbone (csrc/window_attention.hip) ------------------------------------------------
def window_attention(qkv, qkv_bias, bias_table, B, H, W, heads, ws, shift, scale=None):
    """functions.window_attention as torch ops on qkv's device and in its dtype — the contract of dvis_window_attention
    (include/dvis_hip.h), which is what swin.py:235-295 computes around WindowAttention.forward: qkv (B, H W, 3 C) on the unpadded
    grid, columns [3][heads][d]; the token at shifted coordinate (ys, xs) is source ((ys + shift) % Hp, (xs + shift) % Wp), a source
    at or beyond (H, W) is a pad token with q / k / v = qkv_bias (zeros when None); per window and head softmax(scale q k^T +
    table[relative position] - 100 [regions differ, shift > 0]) v; rows are written at un-padded sources only -> (B, H W, C)."""
    C = qkv.shape[-1] // 3
    d, N, dev = C // heads, ws * ws, qkv.device
    scale = d ** -0.5 if scale is None else scale
    nh, nw = -(-H // ws), -(-W // ws)
    Hp, Wp = nh * ws, nw * ws
    ys, xs = torch.arange(Hp, device=dev), torch.arange(Wp, device=dev)
    sy, sx = (ys + shift) % Hp, (xs + shift) % Wp
    valid = ((sy < H)[:, None] & (sx < W)[None, :]).reshape(-1)                                  # per shifted coordinate
    src = torch.where(valid, (sy[:, None] * W + sx[None, :]).reshape(-1), torch.full((), H * W, device=dev))
    pad = qkv.new_zeros(3 * C) if qkv_bias is None else qkv_bias.to(qkv.dtype)
    rows = torch.cat([qkv.reshape(B, H * W, 3 * C), pad.expand(B, 1, 3 * C)], dim=1)[:, src]     # (B, Hp Wp, 3 C), shifted order
    q, k, v = rows.view(B, nh, ws, nw, ws, 3, heads, d).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, B, nh * nw, heads, N, d)
    attn = (q * scale) @ k.transpose(-2, -1)                                                      # (B, nW, heads, N, N)
    ly, lx = torch.arange(N, device=dev) // ws, torch.arange(N, device=dev) % ws
    index = (ly[:, None] - ly[None, :] + ws - 1) * (2 * ws - 1) + (lx[:, None] - lx[None, :] + ws - 1)
    attn = attn + bias_table.to(qkv.dtype)[index.reshape(-1)].view(N, N, heads).permute(2, 0, 1)
    if shift > 0:
        r = lambda n, size: (n >= size - ws).long() + (n >= size - shift).long()
        region = (3 * r(ys, Hp)[:, None] + r(xs, Wp)[None, :]).view(nh, ws, nw, ws).permute(0, 2, 1, 3).reshape(nh * nw, N)
        differ = region[:, :, None] != region[:, None, :]
        attn = attn + torch.where(differ, -100.0, 0.0).to(qkv.dtype)[None, :, None]
    o = torch.softmax(attn, dim=-1) @ v                                                           # (B, nW, heads, N, d)
    o = o.view(B, nh, nw, heads, ws, ws, d).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, Hp * Wp, C)
    out = qkv.new_empty(B, H * W, C)
    out[:, src[valid]] = o[:, valid]
    return out


# --- first half of a ConvNeXt block (csrc/dwconv_ln.hip) ---------------------------------------------------------------------------
def dwconv7x7_ln_tokens(x, conv_dw, norm, hw=None):
    """functions.dwconv7x7_ln_tokens as torch ops on x's device and in its dtype: the token-major map x (B, h, w, C) (or (B, h w, C)
    with hw = (h, w)) goes to NCHW, through the depthwise convolution, back to NHWC and through the LayerNorm over C — timm's
    ConvNeXtBlock up to mlp.fc1 -> a tensor of x's shape."""
    B = x.shape[0]
    h, w = (x.shape[1], x.shape[2]) if hw is None else (int(hw[0]), int(hw[1]))
    C = x.shape[-1]
    z = F.conv2d(x.reshape(B, h, w, C).permute(0, 3, 1, 2), conv_dw.weight.to(x.dtype),
                 None if conv_dw.bias is None else conv_dw.bias.to(x.dtype), stride=1, padding=3, groups=C)
    y = F.layer_norm(z.permute(0, 2, 3, 1), (C,), norm.weight.to(x.dtype), norm.bias.to(x.dtype), norm.eps)
    return y.reshape(x.shape)


def causal_self_attention(qkv, heads, attn_mask):
    """The self-attention of CLIP's text tower as plain torch ops, on any device: qkv (N, L, 3 D) = the block's in-projection, columns
    [3][heads][d]; attn_mask (L, L) additive (-inf above the diagonal) -> (N, L, D), ready for the out-projection.  This is NOT a hot
    path: the tower runs once per vocabulary on 77 tokens and the meta-architecture caches its result, so there is no kernel for it."""
    N, L, D3 = qkv.shape
    d = D3 // 3 // heads
    q, k, v = qkv.view(N, L, 3, heads, d).permute(2, 0, 3, 1, 4)
    a = torch.softmax((q * d ** -0.5) @ k.transpose(-1, -2) + attn_mask.to(qkv.dtype), dim=-1)
    return (a @ v).permute(0, 2, 1, 3).reshape(N, L, heads * d)


# --- classification of the open-vocabulary (FC-CLIP) heads (csrc/mask_pool.hip, csrc/ov_class_logits.hip) ---------------------------
def mask_pool(x, mask_logits):
    """functions.mask_pool as torch ops: x (B, C, H, W), mask_logits (B, Q, H, W) (any strides) -> (sum (B, Q, C) of x over the pixels
    with logit > 0 — false for 0.0, -0.0 and NaN —, count (B, Q) int32 of those pixels): MaskPooling
    (ov_dvis/video_mask2former_transformer_decoder_ov.py:39-67) before its division."""
    inside = mask_logits > 0
    return torch.einsum("bchw,bqhw->bqc", x, inside.to(x.dtype)), inside.sum(dim=(-1, -2)).to(torch.int32)


def text_class_logits(x, text_classifier, logit_scale, num_templates):
    """get_classification_logits (ov_dvis/video_mask2former_transformer_decoder_ov.py:17-36) for x (..., D): normalise, scale by
    min(exp(logit_scale), 100), multiply by text_classifier (N, D)^T and take the maximum over each group's templates ->
    (..., len(num_templates)).  The groups are consecutive (the caller checked that they add up to N: the reference's "last n rows"
    for the void group is then the same rows)."""
    scale = torch.clamp(logit_scale.to(x.dtype).exp(), max=100)
    logits = (scale * F.normalize(x, dim=-1)) @ text_classifier.to(x.dtype).T
    return torch.stack([part.max(-1).values for part in logits.split([int(n) for n in num_templates], dim=-1)], dim=-1)


def ov_ensemble(in_logits, out_logits, overlapping, alpha, beta, valid=None):
    """The geometric ensemble of ov_dvis/meta_architecture_ov.py:603-642 on rows (..., K + 1), in the log domain (the contract of
    dvis_ov_ensemble, include/dvis_hip.h): c_k = (1 - a_k) log_softmax(in[:K])_k + a_k log_softmax(out[:K])_k with a_k = alpha where
    overlapping_k else beta, times (valid > 0) when given; -> log(cat(softmax(c) (1 - p_void), p_void) + 1e-8), p_void the softmax
    of all K + 1 in-vocabulary logits at the last one."""
    dt = in_logits.dtype
    seen = overlapping.to(in_logits.device) != 0
    a = torch.where(seen, torch.tensor(float(alpha), dtype=dt), torch.tensor(float(beta), dtype=dt))
    if valid is not None:
        a = a * (valid > 0).to(dt).unsqueeze(-1)
    c = (1 - a) * torch.log_softmax(in_logits[..., :-1], -1) + a * torch.log_softmax(out_logits[..., :-1].to(dt), -1)
    p_void = torch.softmax(in_logits, -1)[..., -1:]
    return torch.log(torch.cat([torch.softmax(c, -1) * (1.0 - p_void), p_void], dim=-1) + 1e-8)
