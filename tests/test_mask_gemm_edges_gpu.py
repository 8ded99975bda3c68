"""GPU: the mask-logit kernels (csrc/mask_gemm.hip: mask_logits, attn_mask, attn_mask_pooled, center_pool3) at their multi-step,
dispatch, layout and sign edges, on the exact-integer cases of mask_gemm_cases.py.

Every comparison is torch.equal against the reference project's op sequence in fp64 on the CPU (einsum -> F.interpolate(bilinear,
align_corners=False) -> sigmoid() < 0.5): logits, mask bytes and allowed_count, with no "decided" filter and no tolerance — the
inputs make every intermediate exact in fp32 (mask_gemm_cases.py says why and asserts it before anything goes to the GPU).  Every
case first asserts its own plan through Fn.mask_gemm_plan, the function the launch consults, so a case that claims an edge fails
loudly when a later change moves the edge.

The multi-step cases are the only op-level tests in which a workgroup runs more than one step (total_steps > nwg): the step loop,
the prefetch of the next step's first map fragments under the last MFMAs, the frame change inside a workgroup's share with its
reload of mask_embed, and the flush of the per-row counts on that change.
"""
import ctypes

import pytest
import torch

import mask_gemm_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

QT_OF = {1: (2,), 16: (2,), 17: (2,), 32: (2,), 33: (4,), 64: (4,), 65: (7,), 112: (7,), 113: (4, 4), 129: (7, 4), 224: (7, 7),
         225: (7, 7, 7), 256: (7, 7, 4)}


def _fn():
    from dvis_plus_amd import functions as Fn
    return Fn


def _plan(mode, e, f, size=None, **kw):
    """The plan of the call op(e, f, size), from the tensors' shapes."""
    B, Q, C = e.shape
    return _fn().mask_gemm_plan(mode, B, Q, C, f.shape[2], f.shape[3], *(size or (0, 0)), **kw)


def _values(mode, case, size=None):
    """fp64 logits (B, Q, pixels) of the case's op in the reference's op sequence: mode 0 the einsum, modes 1 and 2 the down-sized
    logits the mask is the sign of (mode 2: of a pooled map, which the resize to its own size leaves as it is)."""
    if mode == 0:
        v = MC.reference_logits(case.embed, case.feat).flatten(2)
    else:
        v = MC.reference_small(case.embed, case.feat, size if mode == 1 else case.feat.shape[2:])
    MC.assert_exact_outputs(v)
    return v


def _run(mode, e, f, size=None):
    Fn = _fn()
    if mode == 0:
        return (Fn.mask_logits(e, f).flatten(2),)
    return Fn.attn_mask(e, f, size) if mode == 1 else Fn.attn_mask_pooled(e, f)


def _assert_mask(mask, allowed, rmask, rcount=None):
    mask, allowed = mask.cpu(), allowed.cpu()
    assert mask.dtype == torch.uint8 and allowed.dtype == torch.int32
    assert torch.equal(mask, rmask.to(torch.uint8))
    assert torch.equal(allowed, (mask == 0).sum(-1).to(torch.int32))
    assert torch.equal(allowed, (~rmask).sum(-1).to(torch.int32) if rcount is None else rcount)


def _check(mode, e, f, size, values):
    """Run the op on GPU tensors and compare the whole output with the reference; returns the outputs."""
    out = _run(mode, e, f, size)
    if mode == 0:
        assert torch.equal(out[0].cpu(), values.float())
    else:
        _assert_mask(*out, *MC.reference_mask(values))
    return out


def _check_case(mode, case, size=None, frames=()):
    e, f = case.embed.to(DEV), case.feat.to(DEV)
    out = _check(mode, e, f, size, _values(mode, case, size))
    _check_frames_alone(mode, e, f, size, out, frames)
    return out


def _check_frames_alone(mode, e, f, size, out, frames):
    """Frame b of the batched call has the bits of that frame run alone."""
    for b in frames:
        alone = _run(mode, e[b:b + 1].clone(), f[b:b + 1].clone(), size)
        for a, o in zip(alone, out):
            assert torch.equal(a, o[b:b + 1]), b


def _misaligned(t):
    """A contiguous GPU copy of t that starts 4 bytes into a 16-byte aligned buffer."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---------------------------------------------------------------------------------------------------------------
# multi-step, frame change, prefetch
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MC.MULTI_STEP))
def test_multi_step(name):
    mode, B, Q, C, H, W, size, want = MC.MULTI_STEP[name]
    case = MC.multi_step_case(name)
    p = _plan(mode, case.embed, case.feat, size)
    print(name, [f"total_steps={x.total_steps} nwg={x.nwg}" for x in p])
    assert [(x.QT, x.spf, x.total_steps, x.nwg) for x in p] == want
    assert p[0].total_steps > p[0].nwg
    assert all(x.fullc == (C % 32 == 0) and x.vec == (mode != 1 and C % 32 == 0 and H * W % 4 == 0) for x in p)
    _check_case(mode, case, size, frames=(0, B // 2, B - 1))


def test_pooled_byte_stores_at_130_frames():
    """attn_mask_pooled at (130, 100, 32, 15, 7): HW % 4 != 0 (byte stores).  One step per frame: 130 steps on 130 workgroups, so
    this shape is a single-step launch; MULTI_STEP["pooled_byte_stores"] is the same at B = 260."""
    mode, B, Q, C, h, w, _, want = MC.POOLED_BYTE_STORES_130
    case = MC.make_case(B, Q, C, h, w, seed=130, quarters=True)
    p = _plan(mode, case.embed, case.feat)
    assert [(x.QT, x.spf, x.total_steps, x.nwg) for x in p] == want and not p[0].vec
    _check_case(mode, case, frames=(0, B // 2, B - 1))


def test_multi_step_pooled_through_center_pool3():
    """attn_mask_pooled on the s = 8 level of center_pool3 of a (130, 32, 128, 288) map: 16 x 36 pixels, 9 groups and 2 steps per
    frame, 260 steps on 256 workgroups, 16-byte loads and packed stores."""
    Fn = _fn()
    mode, B, Q, C, h, w, _, want = MC.POOLED_VEC
    case = MC.pooled_vec_case()
    e, f = case.embed.to(DEV), case.feat.to(DEV)
    with torch.no_grad():
        p8, _, _ = Fn.center_pool3(f)
    del f
    assert p8.shape == (B, C, h, w)
    (p,) = _plan(mode, e, p8)
    print("pooled_vec", f"total_steps={p.total_steps} nwg={p.nwg}")
    assert [(p.QT, p.spf, p.total_steps, p.nwg)] == want and p.total_steps > p.nwg and p.vec and p.fullc and p.gpf == 9
    values = MC.reference_small(case.embed, case.feat, (h, w), chunk=5)
    MC.assert_exact_outputs(values)
    out = _check(mode, e, p8, None, values)
    _check_frames_alone(mode, e, p8, None, out, (0, B // 2, B - 1))


# ---------------------------------------------------------------------------------------------------------------
# lattices
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", sorted(QT_OF))
def test_query_lattice(Q):
    B, C, H, W, s = 2, 32, 8, 12, 2
    h, w = H // s, W // s
    case = MC.make_case(B, Q, C, H, W, seed=Q, zero_pixels=MC.center_pixels(H, W, s, h * w - 1))
    pooled = MC.make_case(B, Q, C, h, w, seed=1000 + Q, quarters=True)
    for mode, c, size in ((0, case, None), (1, case, (h, w)), (2, pooled, None)):
        p = _plan(mode, c.embed, c.feat, size)
        assert tuple(x.QT for x in p) == QT_OF[Q] and [x.qbeg for x in p] == MC.passes_of(Q), (mode, p)
        _check_case(mode, c, size, frames=(0, 1))


@pytest.mark.parametrize("C", [32, 64, 256, 1, 3, 4, 5, 31, 33, 100, 255])
def test_channel_lattice(C):
    """65 pixels (one full wave group and one pixel; not a multiple of 4) at every kind of channel count: FULLC (C % 32 == 0), and
    not — C below one k-step, not a multiple of 4, one short of and one past a multiple of 32."""
    B, Q, h, w, s = 2, 33, 5, 13, 2
    small = MC.make_case(B, Q, C, h, w, seed=C)
    big = MC.make_case(B, Q, C, h * s, w * s, seed=300 + C, zero_pixels=MC.center_pixels(h * s, w * s, s, h * w - 1))
    pooled = MC.make_case(B, Q, C, h, w, seed=600 + C, quarters=True)
    for mode, c, size in ((0, small, None), (1, big, (h, w)), (2, pooled, None)):
        (p,) = _plan(mode, c.embed, c.feat, size)
        assert p.fullc == (C % 32 == 0) and not p.vec and p.QT == 4
        _check_case(mode, c, size, frames=(0, 1))


@pytest.mark.parametrize("C", [33, 100, 255])
def test_one_hot_channels_not_fullc(C):
    """The transpose-detecting construction of test_mask_gemm_gpu.py where K is permuted per lane group with a ragged last group:
    every query selects one channel, the features are a distinct integer per (frame, channel, pixel)."""
    B, Q, H, W = 2, 33, 5, 13
    e = torch.zeros(B, Q, C)
    for b in range(B):
        for q in range(Q):
            e[b, q, (q * 7 + 3 + b) % C] = 1.0 + q
    f = torch.arange(B * C * H * W, dtype=torch.float32).reshape(B, C, H, W)
    ref = MC.reference_logits(e, f)
    assert float(ref.max()) < 2 ** 24                       # one non-zero product per output: exact
    assert not _plan(0, e, f)[0].fullc
    assert torch.equal(_fn().mask_logits(e.to(DEV), f.to(DEV)).cpu().double(), ref)


@pytest.mark.parametrize("HW", [1, 3, 4, 63, 64, 65, 511, 512, 513])
def test_pixel_edges_logits(HW):
    case = MC.make_case(2, 17, 32, 1, HW, seed=HW)
    (p,) = _plan(0, case.embed, case.feat)
    assert p.vec == (HW % 4 == 0) and p.gpf == -(-HW // 64) and p.spf == -(-p.gpf // 8)
    _check_case(0, case, frames=(0, 1))


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (1, 16), (1, 17), (7, 17), (8, 16)])
def test_pixel_edges_attn_mask(h, w):
    """Groups of 16 outputs that end inside a row, span rows, or are short; every even factor the decoder or a test uses."""
    for s in (2, 4, 6, 8, 16):
        H, W = h * s, w * s
        case = MC.make_case(2, 17, 32, H, W, seed=100 * s + h * w, zero_pixels=MC.center_pixels(H, W, s, h * w - 1))
        (p,) = _plan(1, case.embed, case.feat, (h, w))
        assert p.gpf == -(-h * w // 16) and not p.vec
        _check_case(1, case, (h, w), frames=(0, 1))


@pytest.mark.parametrize("h,w", [(1, 1), (2, 5), (3, 5), (4, 4), (1, 17), (8, 8), (5, 13)])
def test_pixel_edges_attn_mask_pooled(h, w):
    case = MC.make_case(2, 17, 32, h, w, seed=h * w, quarters=True)
    (p,) = _plan(2, case.embed, case.feat)
    assert p.vec == (h * w % 4 == 0) and p.gpf == -(-h * w // 64)
    _check_case(2, case, frames=(0, 1))


# ---------------------------------------------------------------------------------------------------------------
# alignment
# ---------------------------------------------------------------------------------------------------------------
def test_vec_switched_off_by_the_pointer():
    """HW % 4 == 0 and C % 32 == 0, the map 4 bytes into a buffer: the scalar-load forms run, with the bits of the aligned call."""
    Fn = _fn()
    for mode, quarters in ((0, False), (2, True)):
        case = MC.make_case(2, 33, 32, 8, 8, seed=7 + mode, quarters=quarters)
        assert _plan(mode, case.embed, case.feat)[0].vec and not _plan(mode, case.embed, case.feat, aligned=False)[0].vec
        e, f = case.embed.to(DEV), case.feat.to(DEV)
        want = _check(mode, e, f, None, _values(mode, case))
        got = _run(mode, e, _misaligned(f))
        assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("C", [32, 256])
def test_misaligned_embed_takes_the_scalar_form(C):
    """mask_embed 4 bytes into a buffer: the FULLC forms would read it as 16-byte vectors, so the launch takes the forms that read
    it by scalars (the plan says so) — same bits as the aligned call, in all three modes."""
    B, Q, h, w, s = 2, 33, 4, 8, 2
    big = MC.make_case(B, Q, C, h * s, w * s, seed=C, zero_pixels=MC.center_pixels(h * s, w * s, s, h * w - 1))
    pooled = MC.make_case(B, Q, C, h, w, seed=C + 1, quarters=True)
    for mode, c, size in ((0, big, None), (1, big, (h, w)), (2, pooled, None)):
        (p,) = _plan(mode, c.embed, c.feat, size)
        (pm,) = _plan(mode, c.embed, c.feat, size, embed_aligned=False)
        assert p.fullc and p.vec == (mode != 1) and not pm.fullc and not pm.vec
        e, f = c.embed.to(DEV), c.feat.to(DEV)
        want = _check(mode, e, f, size, _values(mode, c, size))
        got = _run(mode, _misaligned(e), f, size)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), mode


# ---------------------------------------------------------------------------------------------------------------
# guard bands: the C entry points write nothing outside their outputs
# ---------------------------------------------------------------------------------------------------------------
MARGIN = 64
FLOAT_SENTINEL = 0x7FC0BEEF        # a fixed bit pattern (a NaN with a payload): compared as int32
BYTE_SENTINEL = 0xA5               # neither 0 nor 1
COUNT_SENTINEL = -123456789


def _guarded(n, dtype, fill, front=MARGIN):
    buf = torch.full((front + n + MARGIN,), fill, dtype=dtype, device=DEV)
    return buf, buf[front:front + n], ctypes.c_void_p(buf.data_ptr() + front * buf.element_size())


def _assert_margins(buf, n, fill, front=MARGIN):
    assert bool((buf[:front] == fill).all()) and bool((buf[front + n:] == fill).all())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("Q", [17, 113])
def test_guard_bands(Q):
    from dvis_plus_amd import native
    lib, B, C = native.lib(), 2, 32
    stream = native.stream_ptr(torch.device(DEV))
    # mode 0 at HW = 65
    case = MC.make_case(B, Q, C, 5, 13, seed=Q)
    e, f = case.embed.to(DEV), case.feat.to(DEV)
    n = B * Q * 65
    buf, inner, p = _guarded(n, torch.int32, FLOAT_SENTINEL)
    assert lib.dvis_mask_logits(_ptr(e), _ptr(f), B, Q, C, 65, p, stream) == 0
    torch.cuda.synchronize()
    _assert_margins(buf, n, FLOAT_SENTINEL)
    assert torch.equal(inner.view(torch.float32).view(B, Q, 65).cpu(), _values(0, case).float())
    # mode 1 at (7, 17), mode 2 at 3 x 5 with the mask 4 bytes off a 16-byte boundary
    big = MC.make_case(B, Q, C, 14, 34, seed=Q + 1, zero_pixels=MC.center_pixels(14, 34, 2, 7 * 17 - 1))
    pooled = MC.make_case(B, Q, C, 3, 5, seed=Q + 2, quarters=True)
    for mode, c, (h, w), front in ((1, big, (7, 17), MARGIN), (2, pooled, (3, 5), MARGIN + 4)):
        e, f = c.embed.to(DEV), c.feat.to(DEV)
        n = B * Q * h * w
        mbuf, mask, pm = _guarded(n, torch.uint8, BYTE_SENTINEL, front)
        cbuf, count, pc = _guarded(B * Q, torch.int32, COUNT_SENTINEL)
        assert pm.value % 16 == (front - MARGIN)
        if mode == 1:
            rc = lib.dvis_attn_mask(_ptr(e), _ptr(f), B, Q, C, 14, 34, h, w, pm, pc, stream)
        else:
            rc = lib.dvis_attn_mask_pooled(_ptr(e), _ptr(f), B, Q, C, h, w, pm, pc, stream)
        torch.cuda.synchronize()
        assert rc == 0
        _assert_margins(mbuf, n, BYTE_SENTINEL, front)
        _assert_margins(cbuf, B * Q, COUNT_SENTINEL)
        _assert_mask(mask.view(B, Q, h * w), count.view(B, Q), *MC.reference_mask(_values(mode, c, (h, w))))


# ---------------------------------------------------------------------------------------------------------------
# the decision is the sign of the down-sized logit, and nothing else
# ---------------------------------------------------------------------------------------------------------------
def test_sign_only():
    """blocked <=> down-sized logit < 0: a row scaled by 2^-100 or 2^100 (exact, no underflow or overflow at |logit| <= 4096) keeps
    its mask row and its count, and a row of -0.0 is allowed everywhere.  (Compared with the unscaled kernel rows and the fp64 sign,
    not with sigmoid() < 0.5, which rounds to 0.5 at 2^-100.)"""
    B, Q, C, h, w, s = 2, 33, 32, 7, 17, 2
    big = MC.make_case(B, Q, C, h * s, w * s, seed=5, zero_pixels=MC.center_pixels(h * s, w * s, s, h * w - 1))
    pooled = MC.make_case(B, Q, C, h, w, seed=6, quarters=True)
    free = [q for q in range(Q) if q not in MC.planted_positions(Q)]
    down, up, negzero = free[0], free[7], free[20]
    for mode, c, size in ((1, big, (h, w)), (2, pooled, None)):
        values = _values(mode, c, size)
        e, f = c.embed.to(DEV), c.feat.to(DEV)
        mask, count = _check(mode, e, f, size, values)
        e2 = e.clone()
        e2[:, down] *= 2.0 ** -100
        e2[:, up] *= 2.0 ** 100
        e2[:, negzero] = -0.0
        assert bool(torch.isfinite(e2).all()) and bool((e2[:, down].abs() >= 2.0 ** -100)[e[:, down] != 0].all())
        mask2, count2 = _run(mode, e2, f, size)
        rows = [q for q in range(Q) if q != negzero]
        assert torch.equal(mask2[:, rows], mask[:, rows]) and torch.equal(count2[:, rows], count[:, rows])
        sign = (values < 0).to(torch.uint8)
        assert torch.equal(mask2[:, [down, up]].cpu(), sign[:, [down, up]])
        assert bool(sign[:, [down, up]].any()) and not bool(sign[:, [down, up]].all())
        assert not bool(mask2[:, negzero].any()) and bool((count2[:, negzero] == h * w).all())


@pytest.mark.parametrize("C", [32, 33])
def test_one_nan_feature(C):
    """One NaN in the features of frame 0 (last channel, one pixel): mask_logits is NaN at exactly that pixel of every query row of
    frame 0; attn_mask / attn_mask_pooled report the output it feeds as allowed (NaN < 0 is false); everything else is untouched."""
    Fn = _fn()
    B, Q, h, w, s = 2, 17, 8, 8, 2
    o = 37                                                                          # the affected output pixel
    small = MC.make_case(B, Q, C, h, w, seed=C)
    big = MC.make_case(B, Q, C, h * s, w * s, seed=C + 1, zero_pixels=MC.center_pixels(h * s, w * s, s, h * w - 1))
    pooled = MC.make_case(B, Q, C, h, w, seed=C + 2, quarters=True)
    keep = [p for p in range(h * w) if p != o]
    # mode 0
    f = small.feat.clone()
    f[0, C - 1].view(-1)[o] = float("nan")
    out = Fn.mask_logits(small.embed.to(DEV), f.to(DEV)).flatten(2).cpu()
    assert bool(out[0, :, o].isnan().all()) and int(out.isnan().sum()) == Q
    assert torch.equal(out[:, :, keep], _values(0, small).float()[:, :, keep])
    # modes 1 and 2
    for mode, c, size, pixel in ((1, big, (h, w), MC.center_pixels(h * s, w * s, s, o)[2]), (2, pooled, None, o)):
        f = c.feat.clone()
        f[0, C - 1].view(-1)[pixel] = float("nan")
        rmask, _ = MC.reference_mask(_values(mode, c, size))
        rmask[0, :, o] = False
        _assert_mask(*_run(mode, c.embed.to(DEV), f.to(DEV), size), rmask)


def test_refusals():
    Fn = _fn()
    e, f = torch.zeros(1, 4, 257, device=DEV), torch.zeros(1, 257, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="C <= 256"):
        Fn.mask_logits(e, f)
    with pytest.raises(RuntimeError, match="C <= 256"):
        Fn.attn_mask(e, f, (4, 4))
    with pytest.raises(RuntimeError, match="C <= 256"):
        Fn.attn_mask_pooled(e, f)
    e, f = torch.zeros(1, 4, 32, device=DEV), torch.zeros(1, 32, 8, 16, device=DEV)
    with pytest.raises(RuntimeError, match="even integer"):
        Fn.attn_mask(e, f, (4, 4))                                                   # H / h = 2, W / w = 4
    with torch.no_grad():
        assert Fn.center_pool3(torch.zeros(1, 8, 16, 20, device=DEV)) is None      # W % 8 != 0
        assert Fn.center_pool3(torch.zeros(1, 8, 16, 24, device=DEV)) is not None
