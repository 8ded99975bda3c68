"""GPU: the second form of the top-down image kernel (csrc/conv1x1_x3.hip: upsample_add_image_v2_kernel — 16-byte lateral loads, the
block's top taps staged once in LDS, fragments transposed through LDS) and the token-major `top` operand
(dvis_upsample_add_image_tokens) against the first form, which stays in the library and is the reference here.

Pinned: equal image BYTES (padding pixels of a row's last group included) for every shape, with and without the GroupNorm affine,
with `top` as an (N, C, h, w) map and as token-major rows at row0 > 0 of a longer (N, S, C) tensor; the decoded image against the
torch expression; W % 4 != 0 falls back to the first form; run-to-run bits; a frame's bytes independent of the batch.

Bound against torch (fp64), two terms.  Values: an image element carries 22 bits (hi + lo, 11 + 11) and the fp32 evaluation rounds
five times at 2^-24 of the largest intermediate: 2^-21 max|torch| (the bound tests/test_conv_image_gpu.py uses for the first form at
2 x, where the coordinates are exact).  Coordinates: the kernels evaluate fx = sx (x + 0.5) - 0.5 in fp32 — sx = w / W rounded once
(2^-24 relative, on a value below w) and the fused multiply-add once more — so fx is off by at most 2^-23 w, fy by 2^-23 h, and a
bilinear sum moves by that times the largest difference of neighbouring top values along the axis: 2^-23 (w Dx + h Dy)."""
import pytest
import torch
import torch.nn.functional as F

from test_conv_image_gpu import decode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [
    (2, 64, 6, 40, 3, 20),          # one full group plus 8 pixels
    (3, 128, 17, 36, 9, 18),        # odd H, non-integer row scale, H not a multiple of the row block
    (1, 256, 24, 160, 12, 80),      # the 96 x 160 test pyramid
    (2, 64, 5, 4, 3, 2),            # a single partial group
    (2, 64, 8, 132, 4, 66),         # four groups plus 4 pixels
]


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


class first_form:
    """The first kernel form for the calls inside (dvis_upsample_add_image_set_v2)."""

    def __enter__(self):
        from dvis_plus_amd import native
        self.prev = native.lib().dvis_upsample_add_image_set_v2(0)

    def __exit__(self, *exc):
        from dvis_plus_amd import native
        native.lib().dvis_upsample_add_image_set_v2(self.prev)


def _bound(want, top):
    """The module docstring's bound on |decoded image - torch fp64| for these operands."""
    h, w = top.shape[-2:]
    dx = float((top[..., :, 1:] - top[..., :, :-1]).abs().max()) if w > 1 else 0.0
    dy = float((top[..., 1:, :] - top[..., :-1, :]).abs().max()) if h > 1 else 0.0
    return 2.0 ** -21 * float(want.abs().max()) + 2.0 ** -23 * (w * dx + h * dy)


_CASES = {}


def case(shape, affine):
    """Operands of a shape and the first form's image of them: made once, shared, never written."""
    key = (shape, affine)
    if key not in _CASES:
        from dvis_plus_amd import functions as Fn
        N, C, H, W, h, w = shape
        g = torch.Generator().manual_seed(1000 * H + W + int(affine))
        lat = torch.randn(N, C, H, W, generator=g).to(DEV)
        row0, tail = 7, 5                                   # the level's rows inside a longer token matrix
        tokens = torch.randn(N, row0 + h * w + tail, C, generator=g).to(DEV)
        top = tokens[:, row0:row0 + h * w].transpose(1, 2).reshape(N, C, h, w)      # the token-major view
        aff = (torch.rand(N * C, generator=g).to(DEV) + 0.5, torch.randn(N * C, generator=g).to(DEV)) if affine else None
        with first_form():
            ref = Fn.upsample_add_image(lat, top.contiguous(), aff)
        _CASES[key] = (lat, top, aff, ref)
    return _CASES[key]


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_second_form_writes_the_first_forms_bytes(shape, affine):
    from dvis_plus_amd import functions as Fn, native
    N, C, H, W, h, w = shape
    lat, top, aff, ref = case(shape, affine)
    assert native.lib().dvis_upsample_add_image_v2_supported(N, C, H, W, h, w)
    assert native.lib().dvis_upsample_add_image_set_v2(-1) == 1
    got = Fn.upsample_add_image(lat, top.contiguous(), aff)            # top as a map
    assert torch.equal(got.data, ref.data)
    assert Fn.upsample_add_image_reads_tokens(lat, top)
    tok = Fn.upsample_add_image(lat, top, aff)                         # top as token-major rows at row0 > 0
    assert torch.equal(tok.data, ref.data)
    assert torch.equal(Fn.upsample_add_image(lat, top, aff).data, tok.data)      # run to run
    # against torch
    l64 = lat.double()
    if aff is not None:
        l64 = l64 * aff[0].double().view(N, C, 1, 1) + aff[1].double().view(N, C, 1, 1)
    want = l64 + F.interpolate(top.double(), size=(H, W), mode="bilinear", align_corners=False)
    bound = _bound(want, top)
    for img in (got, tok, ref):
        err = float((decode(img).double() - want).abs().max())
        print(f"{shape} affine={affine}: max|decoded - torch| {err:.3e} (bound {bound:.3e})")
        assert err <= bound


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]])
def test_a_frames_bytes_do_not_depend_on_the_batch(shape):
    from dvis_plus_amd import functions as Fn
    N, C, H, W, h, w = shape
    lat, top, aff, ref = case(shape, True)
    per = ref.data.numel() // N
    for n in range(N):
        a = (aff[0].view(N, C)[n].contiguous(), aff[1].view(N, C)[n].contiguous())
        one = Fn.upsample_add_image(lat[n:n + 1], top[n:n + 1], a)
        assert Fn.upsample_add_image_reads_tokens(lat[n:n + 1], top[n:n + 1])
        assert torch.equal(one.data, ref.data[n * per:(n + 1) * per])
        one = Fn.upsample_add_image(lat[n:n + 1], top[n:n + 1].contiguous(), a)
        assert torch.equal(one.data, ref.data[n * per:(n + 1) * per])


def test_rows_that_are_no_multiple_of_four_pixels_take_the_first_form():
    from dvis_plus_amd import functions as Fn, native
    N, C, H, W, h, w = 2, 64, 6, 38, 3, 19
    assert not native.lib().dvis_upsample_add_image_v2_supported(N, C, H, W, h, w)
    g = torch.Generator().manual_seed(38)
    lat = torch.randn(N, C, H, W, generator=g).to(DEV)
    tokens = torch.randn(N, 3 + h * w, C, generator=g).to(DEV)
    top = tokens[:, 3:].transpose(1, 2).reshape(N, C, h, w)
    assert not Fn.upsample_add_image_reads_tokens(lat, top)
    got = Fn.upsample_add_image(lat, top)                 # (the view is copied to a map)
    with first_form():
        ref = Fn.upsample_add_image(lat, top.contiguous())
    assert torch.equal(got.data, ref.data)
    want = lat.double() + F.interpolate(top.double(), size=(H, W), mode="bilinear", align_corners=False)
    assert float((decode(got).double() - want).abs().max()) <= _bound(want, top)
    with pytest.raises(RuntimeError, match="dvis_upsample_add_image_tokens"):
        data = torch.empty(native.lib().dvis_conv_x3_image_bytes(N, C, H, W), dtype=torch.uint8, device=DEV)
        native.check(native.lib().dvis_upsample_add_image_tokens(
            lat.data_ptr(), None, None, tokens.data_ptr(), tokens.shape[1], 3, data.data_ptr(), N, C, H, W, h, w, 2,
            native.stream_ptr(lat.device)), "dvis_upsample_add_image_tokens")


def test_the_switch_takes_the_first_form():
    from dvis_plus_amd import functions as Fn
    lat, top, aff, ref = case(SHAPES[0], True)
    with first_form():
        assert not Fn.upsample_add_image_reads_tokens(lat, top)
        assert torch.equal(Fn.upsample_add_image(lat, top, aff).data, ref.data)
