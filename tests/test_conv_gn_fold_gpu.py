"""GPU: the GroupNorm folded into the split-f16 convolutions of the pixel decoder's mask path (csrc/conv1x1_x3.hip, FOLD forms;
include/dvis_hip.h: gn_part / in_scale of dvis_conv1x1_x3 and dvis_conv_x3_image, dvis_group_norm_finalize).

Pinned: the convolution's own bits with and without the statistics, (scale, shift) against the separate statistics kernel, a
frame's statistics independent of the batch and of the persistent grid, shapes the folded forms do not serve, the load-path
affine (+ ReLU) bit for bit against the in-place pass followed by the plain launch — the range guard's tag included —, run to run.

Shapes: N = 3 frames of 8 x 36 = 288 pixels = 9 wave slots: one full 256-pixel tile plus a partial one per frame's worth, frames
1 and 2 begin inside a tile.

Tolerance of (scale, shift): 1 fp32 ulp.  Both sides sum the same values in fp64 in different orders: the sums agree to ~1e-16
relative, E[x^2] - E[x]^2 with mean ~ std loses a factor of a few, so rstd and mean agree to ~1e-15 before their ONE rounding to
fp32 — different only when a value lies that close to a rounding boundary; the following fp32 product / subtraction can carry such
a flip, never widen it.  gamma > 0, beta < 0 and a positive mean: shift = beta - mean * scale adds two negative terms, so its ulp
is that of its operands."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, C, K, H, W = 3, 256, 256, 8, 36


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _ulps(a, b):
    """Largest distance of two fp32 tensors of equal signs in units in the last place."""
    assert bool((torch.sign(a) == torch.sign(b)).all())
    return int((a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max())


def _gn(groups=32, seed=5):
    g = torch.Generator().manual_seed(seed)
    gn = torch.nn.GroupNorm(groups, K)
    gn.weight.copy_(0.5 + torch.rand(K, generator=g))          # gamma in [0.5, 1.5]
    gn.bias.copy_(-0.5 - torch.rand(K, generator=g))           # beta in [-1.5, -0.5]
    return gn.to(DEV)


def _operands(taps, n=N, h=H, w=W, seed=11):
    g = torch.Generator().manual_seed(seed + taps)
    k = 3 if taps == 9 else 1
    x = (0.75 + torch.randn(n, C, h, w, generator=g)).to(DEV)                          # non-zero mean
    wt = (torch.randn(K, C, k, k, generator=g) * (1.0 / (C * taps)) ** 0.5).to(DEV)
    b = (1.0 + torch.rand(K, generator=g)).to(DEV)                                     # output mean ~ 1.5, std ~ 1.25
    return x, wt, b


def _image(x):
    from dvis_plus_amd import functions as Fn
    n, c, h, w = x.shape
    return Fn.upsample_add_image(x.contiguous(), torch.zeros(n, c, max(1, h // 2), max(1, w // 2), device=x.device))


def _conv_gn(taps, x, wt, b, gn):
    """(out, (scale, shift)) of the folded form: 1x1 from an fp32 map, 3x3 from an operand image."""
    from dvis_plus_amd import functions as Fn
    if taps == 1:
        return Fn.conv1x1_x3(x, wt, b, gn=gn)
    return Fn.conv_x3_image(_image(x), wt, b, gn=gn)


def _conv(taps, x, wt, b):
    from dvis_plus_amd import functions as Fn
    return Fn.conv1x1_x3(x, wt, b) if taps == 1 else Fn.conv_x3_image(_image(x), wt, b)


@pytest.mark.parametrize("taps", [1, 9])
def test_statistics_from_the_epilogue_match_the_statistics_kernel_and_leave_the_convolution_alone(taps):
    from dvis_plus_amd import functions as Fn
    gn = _gn()
    x, wt, b = _operands(taps)
    assert Fn.PD_GN_FOLD and Fn.gn_fold_ok(gn, K, H * W) and Fn.conv1x1_x3_ok(x, wt)
    plain = _conv(taps, x, wt, b)
    out, (scale, shift) = _conv_gn(taps, x, wt, b, gn)
    Fn.X3_GUARD.check_now(torch.device(DEV))
    assert torch.equal(out, plain)
    ref_scale, ref_shift = Fn.group_norm_affine(plain, gn)
    print("taps", taps, "ulps scale", _ulps(scale, ref_scale), "shift", _ulps(shift, ref_shift))
    assert _ulps(scale, ref_scale) <= 1 and _ulps(shift, ref_shift) <= 1
    # ... and it IS the GroupNorm: against torch in fp64
    want = torch.nn.functional.group_norm(plain.double(), gn.num_groups, gn.weight.double(), gn.bias.double(), gn.eps)
    got = plain.double() * scale.view(N, K, 1, 1).double() + shift.view(N, K, 1, 1).double()
    assert float((got - want).abs().max()) <= 1e-5
    # run to run
    out2, (scale2, shift2) = _conv_gn(taps, x, wt, b, gn)
    assert torch.equal(out2, out) and torch.equal(scale2, scale) and torch.equal(shift2, shift)


@pytest.mark.parametrize("taps", [1, 9])
def test_a_frames_statistics_depend_on_neither_the_batch_nor_the_grid(taps):
    from dvis_plus_amd import functions as Fn, native
    gn = _gn()
    x, wt, b = _operands(taps)
    _, (scale, shift) = _conv_gn(taps, x, wt, b, gn)
    _, (s1, h1) = _conv_gn(taps, x[1:2].contiguous(), wt, b, gn)
    assert torch.equal(s1, scale.view(N, K)[1]) and torch.equal(h1, shift.view(N, K)[1])
    prev = native.lib().dvis_x3_set_reserve(200)          # a persistent grid of 56 workgroups instead of one per CU
    try:
        out_r, (scale_r, shift_r) = _conv_gn(taps, x, wt, b, gn)
    finally:
        native.lib().dvis_x3_set_reserve(prev)
    assert torch.equal(scale_r, scale) and torch.equal(shift_r, shift)
    assert torch.equal(out_r, _conv(taps, x, wt, b))


@pytest.mark.parametrize("h,w,groups", [(5, 7, 32), (H, W, 16)])
def test_unserved_shapes_take_the_statistics_kernel(h, w, groups):
    from dvis_plus_amd import functions as Fn
    gn = _gn(groups)
    assert not Fn.gn_fold_ok(gn, K, h * w)
    for taps in (1, 9):
        x, wt, b = _operands(taps, h=h, w=w)
        out, (scale, shift) = _conv_gn(taps, x, wt, b, gn)
        plain = _conv(taps, x, wt, b)
        ref_scale, ref_shift = Fn.group_norm_affine(plain, gn)
        assert torch.equal(out, plain) and torch.equal(scale, ref_scale) and torch.equal(shift, ref_shift)


@pytest.mark.parametrize("relu", [True, False])
def test_load_path_affine_is_the_in_place_pass_followed_by_the_plain_launch(relu):
    from dvis_plus_amd import functions as Fn
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(23)
    x = torch.randn(N, C, H, W, generator=g).mul(3.0).to(DEV)                          # pre-activation values of both signs
    wt = (torch.randn(K, C, 1, 1, generator=g) * (1.0 / C) ** 0.5).to(DEV)
    b = torch.randn(K, generator=g).to(DEV)
    scale = (torch.randn(N * C, generator=g) * 0.7).to(DEV)                            # per (frame, channel), both signs
    shift = torch.randn(N * C, generator=g).to(DEV)
    assert Fn.affine_in_ok(x, wt)
    Fn.X3_GUARD.check_now(dev)
    want = Fn.conv1x1_x3(Fn.scale_shift_act_(x.clone(), scale, shift, relu=relu), wt, b)
    got = Fn.conv1x1_x3(x, wt, b, affine=(scale, shift), affine_relu=relu)
    Fn.X3_GUARD.check_now(dev)                                                         # in range: the guard stays silent
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)
    assert torch.equal(got, Fn.conv1x1_x3(x, wt, b, affine=(scale, shift), affine_relu=relu))       # run to run
    # one operand inside the split window as stored (9000 < 16380) and beyond it once the affine is applied (x 2: 18000)
    x[1, 5, 3, 7] = 9000.0
    scale[1 * C + 5], shift[1 * C + 5] = 2.0, 0.0
    word = Fn.X3_GUARD.word(dev)
    tags = []
    for fused in (False, True):
        if fused:
            Fn.conv1x1_x3(x, wt, b, affine=(scale, shift), affine_relu=relu)
        else:
            Fn.conv1x1_x3(Fn.scale_shift_act_(x.clone(), scale, shift, relu=relu), wt, b)
        tags.append(int(word.item()))
        word.zero_()
    assert tags[0] != 0 and tags[1] == tags[0], tags
    assert "conv1x1 kernel" in Fn.X3_GUARD.describe(tags[1])
