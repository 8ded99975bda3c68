"""The Swin backbone without a GPU: the reference's state dict, both g21 fixtures (the reference's own D2SwinTransformer) on CPU
tensors, the torch formulation of the window-attention contract against the literal roll / pad / partition / mask composition, and
the errors the module and the library raise."""
import ctypes
import json
import os

import pytest
import torch

import swin_cases as S
from dvis_plus_amd import cpu_ops, d2, functions as Fn, native


@pytest.mark.parametrize("name", S.FIXTURES)
def test_state_dict_keys_and_shapes_equal_the_reference(name):
    with open(os.path.join(S.GOLDEN, "ref_state_shapes_swin.json")) as f:
        want = json.load(f)[name]
    m = d2.build_backbone(S.swin_cfg(S.FIXTURE_SPECS[name][0]), None)
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    assert any(k.endswith("relative_position_index") for k in got)          # persistent buffers: strict=True loads
    assert m.size_divisibility == 32
    shape = m.output_shape()
    assert {k: (v.channels, v.stride) for k, v in shape.items()} == {"res2": (32, 4), "res3": (64, 8), "res4": (128, 16), "res5": (256, 32)}


def test_out_features_filter():
    m = S.fill_weights(d2.build_backbone(S.swin_cfg(7, OUT_FEATURES=["res3", "res5"]), None)).eval()
    with torch.no_grad():
        out = m(S.fixture_image("g21_swin_w7")[:1])
    assert list(out) == ["res3", "res5"] and list(m.output_shape()) == ["res3", "res5"]


@pytest.mark.parametrize("name", S.FIXTURES)
def test_fixture_on_cpu_tensors(name):
    fx = S.fixture(name)
    got = S.run_with_blocks(fx.build(), fx.image)
    assert sorted(got) == sorted(fx.outs)
    for k, want in fx.outs.items():
        print(f"{name} {k}: max |diff| {(got[k] - want).abs().max().item():.3e} (max |value| {fx.meta['max_abs'][k]:.3f})")
        torch.testing.assert_close(got[k], want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape", S.CPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("shifted", [False, True])
def test_formulation_equals_the_literal_composition_fp64(shape, shifted):
    """Both are the same sums in the same order; 1e-12 leaves room for a matmul blocked by another batch shape only (fp64 eps
    2.2e-16 on scores and outputs of order 1 to 10)."""
    H, W, ws, heads, C = shape
    B, shift = 2, ws // 2 if shifted else 0
    qkv, bias, table = (t.double() for t in S.attention_inputs(B, H, W, heads, ws, d=C // heads, seed=H + W))
    want = S.literal_window_attention(qkv, bias, table, B, H, W, heads, ws, shift)
    got = cpu_ops.window_attention(qkv, bias, table, B, H, W, heads, ws, shift)
    assert got.shape == want.shape == (B, H * W, C)
    torch.testing.assert_close(got, want, rtol=0, atol=1e-12)
    assert torch.equal(Fn.window_attention(qkv, bias, table, B, H, W, heads, ws, shift), got)      # CPU tensors dispatch there
    none = cpu_ops.window_attention(qkv, None, table, B, H, W, heads, ws, shift)
    torch.testing.assert_close(none, S.literal_window_attention(qkv, None, table, B, H, W, heads, ws, shift), rtol=0, atol=1e-12)
    if H % ws or W % ws:
        assert not torch.equal(none, got)           # pad tokens carry the bias: they matter


def test_ape_raises_naming_the_key():
    with pytest.raises(NotImplementedError, match="MODEL.SWIN.APE"):
        d2.build_backbone(S.swin_cfg(7, APE=True), None)


def test_forward_with_grad_enabled_raises():
    m = S.fill_weights(d2.build_backbone(S.swin_cfg(7), None))
    x = S.fixture_image("g21_swin_w7")[:1]
    for mode in (m.train(), m.eval()):                                  # keyed off grad mode, not self.training
        with pytest.raises(NotImplementedError, match="no window-attention backward.*tracker and refiner stages"):
            mode(x)
    with torch.no_grad():
        a = m.train()(x)
        b = m.eval()(x)
    assert all(torch.equal(a[k], b[k]) for k in a)                      # .train() under no_grad: the inference forward
    m.requires_grad_(False)
    assert all(torch.equal(m(x)[k], b[k]) for k in b)                   # frozen: nothing to differentiate


def test_minvis_train_with_swin_raises():
    from dvis_plus_amd.config import build_model
    cfg = S.toy_video_cfg("MinVIS")
    m = build_model(cfg, n_things=2).train()
    frames = [torch.rand(3, 64, 96) * 255 for _ in range(2)]
    with pytest.raises(NotImplementedError, match="no window-attention backward"):
        m([{"image": frames, "height": 64, "width": 96, "instances": []}])


def test_unsupported_window_is_refused_by_the_library():
    lib = native.lib()
    assert lib.dvis_window_attention_supported(7, 32) == 1 and lib.dvis_window_attention_supported(12, 32) == 1
    for ws, d in ((3, 8), (7, 64), (8, 32), (12, 16)):
        assert lib.dvis_window_attention_supported(ws, d) == 0
        # refused ahead of every other check and of the launch: the pointers are never read
        fake = ctypes.c_void_p(64)
        rc = lib.dvis_window_attention(fake, None, fake, fake, 1, 9, 9, 2, d, ws, 0, 1.0, None)
        msg = lib.dvis_last_error().decode()
        assert rc != 0 and f"ws={ws}" in msg and f"d={d}" in msg, (rc, msg)
