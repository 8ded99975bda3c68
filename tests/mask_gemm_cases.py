"""Exact-integer cases for the mask-logit kernels (csrc/mask_gemm.hip), shared by test_mask_gemm_plan_cpu.py and
test_mask_gemm_edges_gpu.py.

Inputs are integer-valued fp32 in [-4, 4] with C <= 256 (a pooled map built on the host: multiples of 0.25 in [-4, 4]), so every
product, every partial sum in any order, every four-pixel average and every pooled value is exact in fp32: |logit| <= 4 * 4 * 256 =
4096 in units of at most 1/4 needs 15 of fp32's 24 bits.  The kernel's result must therefore EQUAL the reference project's op
sequence evaluated in fp64 on the CPU (einsum -> F.interpolate(bilinear, align_corners=False) -> sigmoid() < 0.5,
dvis_Plus/video_mask2former_transformer_decoder.py:363-371): no tolerance and no "decided" filter.

Every case plants, at the query rows where the kernel's tiling has an edge (q in {0, 15, 16, Q - 1}, and qbeg - 1 and qbeg of every
later pass):
  ZERO     an all-zero embed row: every logit is exactly 0, the row is allowed everywhere, its count is h * w
  NEG      the negation of a free (not planted) row of the same frame: the two masks are complements except where the logit is 0
  BLOCKED  a row <= -1 in every channel, in a frame whose features are all >= 1: blocked everywhere, count 0
and a pixel whose features are zero in every channel.  A blocked-everywhere row and an all-zero pixel exclude each other (the
pixel's logit is 0, which is allowed), so frames alternate: even frames are SIGNED (features in [-4, 4], the zero pixel, ZERO / NEG
rows), odd frames POSITIVE (features in [1, 4], BLOCKED / ZERO / NEG rows).  The kind planted at a position rotates with the frame,
so over a few frames every position carries every kind.  Where no free row would be left (Q = 1) only even frames are planted, with
ZERO, and every frame is SIGNED.
"""
import collections

import torch
import torch.nn.functional as F

ZERO, NEG, BLOCKED = "zero", "neg", "blocked"
LIMIT = 4          # |embed|, |features| <= LIMIT
MAX_C = 256

Case = collections.namedtuple("Case", "embed feat planted partner zero_pixels signed")
# embed (B, Q, C), feat (B, C, H, W) fp32 on the CPU; planted: {(b, q): kind}; partner: {(b, q): the free row NEG negates};
# zero_pixels: flat indices into H * W of the all-zero pixels of the SIGNED frames; signed: per frame, whether it is SIGNED


def passes_of(Q):
    """First query of every pass over the queries — what mask_gemm_plan reports as qbeg (test_mask_gemm_plan_cpu.py pins that the
    two agree)."""
    tiles = -(-Q // 16)
    passes = -(-tiles // 7)
    per_pass = -(-tiles // passes)
    return [p * per_pass * 16 for p in range(passes)]


def planted_positions(Q):
    want = {0, 15, 16, Q - 1}
    for qbeg in passes_of(Q)[1:]:
        want |= {qbeg - 1, qbeg}
    return sorted(q for q in want if 0 <= q < Q)


def center_pixels(H, W, s, o):
    """Flat indices of the four centre pixels of block `o` (flat, of the (H / s, W / s) output) of an H x W map: the taps of the
    bilinear down-sizing by the even factor s."""
    oi, oj = divmod(o, W // s)
    y, x = oi * s + s // 2 - 1, oj * s + s // 2 - 1
    return [y * W + x, y * W + x + 1, (y + 1) * W + x, (y + 1) * W + x + 1]


def make_case(B, Q, C, H, W, seed, zero_pixels=None, quarters=False):
    """A case on a (B, C, H, W) map.  zero_pixels: flat pixel indices zeroed in every channel of the SIGNED frames (default: the last
    pixel).  quarters: the map takes multiples of 0.25 — a pooled map built on the host."""
    g = torch.Generator().manual_seed(seed)
    embed = torch.randint(-LIMIT, LIMIT + 1, (B, Q, C), generator=g, dtype=torch.int8).float()
    if quarters:
        feat = torch.randint(-4 * LIMIT, 4 * LIMIT + 1, (B, C, H, W), generator=g, dtype=torch.int8).float() * 0.25
    else:
        feat = torch.randint(-LIMIT, LIMIT + 1, (B, C, H, W), generator=g, dtype=torch.int8).float()
    zero_pixels = [H * W - 1] if zero_pixels is None else list(zero_pixels)
    positions = planted_positions(Q)
    free = [q for q in range(Q) if q not in positions]
    planted, partner, signed = {}, {}, []
    for b in range(B):
        positive = bool(free) and b % 2 == 1
        signed.append(not positive)
        if positive:
            feat[b] = feat[b].abs().clamp_(min=1)
        else:
            feat[b].flatten(1)[:, zero_pixels] = 0
        if not free and b % 2 == 1:
            continue
        kinds = (BLOCKED, ZERO, NEG) if positive else (ZERO, NEG)
        for i, q in enumerate(positions):
            kind = kinds[(i + b // 2) % len(kinds)] if free else ZERO
            planted[(b, q)] = kind
            if kind == ZERO:
                embed[b, q] = 0
            elif kind == BLOCKED:
                embed[b, q] = -embed[b, q].abs().clamp_(min=1)
            else:
                partner[(b, q)] = free[(i + b) % len(free)]
                embed[b, q] = -embed[b, partner[(b, q)]]
    case = Case(embed, feat, planted, partner, zero_pixels, signed)
    assert_exact_inputs(case, quarters)
    return case


def assert_exact_inputs(case, quarters=False):
    """The exactness bound, checked on the CPU before anything is sent to the GPU."""
    e, f = case.embed, case.feat
    assert e.dtype == f.dtype == torch.float32 and e.shape[2] == f.shape[1] <= MAX_C
    assert torch.equal(e, e.round()) and float(e.abs().max()) <= LIMIT
    unit = 4.0 if quarters else 1.0
    assert torch.equal(f * unit, (f * unit).round()) and float(f.abs().max()) <= LIMIT


def reference_logits(embed, feat):
    """einsum("bqc,bchw->bqhw") in fp64."""
    return torch.einsum("bqc,bchw->bqhw", embed.double(), feat.double())


def reference_small(embed, feat, size, chunk=8):
    """The reference's down-sized logits (B, Q, h * w) in fp64: einsum -> F.interpolate(bilinear, align_corners=False), a few
    frames at a time (the full-size logits of a large case never exist at once)."""
    out = []
    for b0 in range(0, embed.shape[0], chunk):
        logits = reference_logits(embed[b0:b0 + chunk], feat[b0:b0 + chunk])
        out.append(F.interpolate(logits, size=tuple(size), mode="bilinear", align_corners=False).flatten(2))
    return torch.cat(out)


def reference_mask(small):
    """(mask bool (B, Q, h * w) with True = blocked, allowed_count int32 (B, Q)) of down-sized fp64 logits."""
    mask = small.sigmoid() < 0.5
    return mask, (~mask).sum(-1).to(torch.int32)


def assert_exact_outputs(values):
    """The reference's fp64 values are fp32 numbers within the bound: the comparison with the kernel can be torch.equal."""
    assert float(values.abs().max()) <= LIMIT * LIMIT * MAX_C
    assert torch.equal(values.float().double(), values) and torch.equal(values * 4, (values * 4).round())


def assert_planted(case, values):
    """The planted rows and pixels do what they were planted for.  values: fp64 logits of the case, (B, Q, pixels) — full size or
    down-sized (then case.zero_pixels do not apply and the caller names the zero outputs itself)."""
    mask, count = reference_mask(values)
    npx = values.shape[-1]
    kinds = set()
    for (b, q), kind in case.planted.items():
        kinds.add(kind)
        if kind == ZERO:
            assert not values[b, q].any() and not mask[b, q].any() and count[b, q] == npx
        elif kind == BLOCKED:
            assert mask[b, q].all() and count[b, q] == 0
        else:
            r = case.partner[(b, q)]
            assert torch.equal(values[b, q], -values[b, r])
            nonzero = values[b, q] != 0
            assert torch.equal(mask[b, q][nonzero], ~mask[b, r][nonzero]) and not (mask[b, q] | mask[b, r])[~nonzero].any()
    return kinds


def assert_multi_frame(case, values, zero_outputs):
    """Every multi-frame case: an exact-zero logit outside the planted rows (here: at `zero_outputs` of every free row of the SIGNED
    frames), and both signs in every frame that has a free row."""
    B, Q = values.shape[:2]
    assert B > 1
    free_zero = 0
    for b in range(B):
        free = [q for q in range(Q) if (b, q) not in case.planted]
        if not free:
            continue
        v = values[b, free]
        assert bool((v < 0).any()) and bool((v > 0).any()), b
        free_zero += int((v == 0).sum())
        if case.signed[b]:
            assert not v[:, zero_outputs].any(), b
    assert free_zero > 0


# ---- the multi-step cases of test_mask_gemm_edges_gpu.py: name -> (mode, B, Q, C, H, W, (h, w) or None, plan per pass as
# (QT, spf, total_steps, nwg)).  H x W is the map the op is given (mode 2: the pooled map).
MULTI_STEP = {
    "logits_shares_cross_frames": (0, 40, 100, 32, 80, 80, None, [(7, 13, 520, 256)]),
    "logits_short_last_step": (0, 130, 100, 32, 24, 24, None, [(7, 2, 260, 256)]),
    "logits_frame_change_every_step": (0, 520, 20, 32, 8, 8, None, [(2, 1, 520, 512)]),
    "logits_two_passes_not_fullc": (0, 70, 129, 40, 48, 48, None, [(7, 5, 350, 256), (4, 5, 350, 350)]),
    "attn_mask_counts_over_workgroups": (1, 70, 100, 32, 32, 64, (16, 32), [(7, 4, 280, 256)]),
    "attn_mask_two_tiles": (1, 130, 20, 32, 32, 64, (16, 32), [(2, 4, 520, 512)]),
    "pooled_byte_stores": (2, 260, 100, 32, 15, 7, None, [(7, 1, 260, 256)]),
}
# attn_mask_pooled at (130, 100, 32, 15, 7): one step per frame, 130 steps on 130 workgroups — a single-step launch; the case above
# is the same at B = 260, the smallest batch with more steps than workgroups at one step per frame.
POOLED_BYTE_STORES_130 = (2, 130, 100, 32, 15, 7, None, [(7, 1, 130, 130)])
# attn_mask_pooled at (130, 100, 32, 16, 36) through center_pool3 of a (130, 32, 128, 288) map
POOLED_VEC = (2, 130, 100, 32, 16, 36, None, [(7, 2, 260, 256)])
POOLED_VEC_MAP = (128, 288, 8)


def multi_step_case(name):
    mode, B, Q, C, H, W, size, _ = MULTI_STEP[name]
    seed = sorted(MULTI_STEP).index(name) + 100
    if mode == 1:
        s = H // size[0]
        return make_case(B, Q, C, H, W, seed, zero_pixels=center_pixels(H, W, s, size[0] * size[1] - 1))
    return make_case(B, Q, C, H, W, seed, quarters=mode == 2)


def multi_step_values(name, case):
    """(fp64 logits of the case's op (B, Q, pixels), the output pixels that case.zero_pixels make zero)."""
    mode, B, Q, C, H, W, size, _ = MULTI_STEP[name]
    if mode == 1:
        return reference_small(case.embed, case.feat, size), [size[0] * size[1] - 1]
    return reference_logits(case.embed, case.feat).flatten(2), case.zero_pixels


def pooled_vec_case(B=None):
    """The full-size map of POOLED_VEC (its s = 8 level is the 16 x 36 map) with the four centre pixels of the last block zero."""
    H, W, s = POOLED_VEC_MAP
    _, B0, Q, C, h, w, _, _ = POOLED_VEC
    return make_case(B or B0, Q, C, H, W, 99, zero_pixels=center_pixels(H, W, s, h * w - 1))
