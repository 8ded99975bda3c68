"""csrc/dwconv_ln.hip on the GPU — depthwise 7 x 7 + bias + channel LayerNorm on token-major maps — against the literal torch
composition of convnext_cases.py (grouped conv2d on NCHW, permute, layer_norm) run on the CPU in fp64, at the project's 4 x rule
(`check_4x`: the kernel may be 4 x as far from the fp64 run as the fp32 CPU run of the same composition is; tensors below the sample
floor take SMALL), and the kernel's bit-level properties.

The inputs (convnext_cases.dwconv_ln_inputs) have per-channel scales spread over 1e-3 .. 1e3 and a mean offset of 50.  Figures of
the CPU runs on them (max |err| against fp64, bias on): the literal fp32 run is finite at every shape, and a kernel that took the
variance as E[z^2] - mean^2 would not pass the 4 x rule — asserted by test_convnext_cpu.py::test_variance_shortcut_would_fail:

  (B, h, w, C)        fp32 literal   fp32 shortcut   ratio
  (2, 3, 5, 8)        3.9e-06        7.3e-05         18.6
  (1, 7, 7, 16)       6.6e-06        1.4e-04         20.8
  (2, 9, 13, 100)     1.4e-05        4.1e-04         28.9
  (1, 4, 70, 192)     8.9e-06        3.3e-04         36.7
  (1, 5, 6, 768)      1.0e-05        2.3e-04         21.8
  (2, 4, 5, 1536)     8.6e-06        2.5e-04         28.6
"""
import ctypes
import functools

import pytest
import torch
from torch import nn

import convnext_cases as K
from dvis_plus_amd import functions as Fn, native
from vit_adapter_train_cases import check_4x

pytestmark = pytest.mark.gpu
DEV = "cuda"


def modules(d, device=DEV):
    """(conv_dw, norm) holding the case's parameters in fp32 on `device`."""
    C = d["weight"].shape[0]
    conv = nn.Conv2d(C, C, 7, padding=3, groups=C, bias=d["bias"] is not None)
    norm = nn.LayerNorm(C, eps=K.EPS)
    with torch.no_grad():
        conv.weight.copy_(d["weight"])
        if d["bias"] is not None:
            conv.bias.copy_(d["bias"])
        norm.weight.copy_(d["gamma"])
        norm.bias.copy_(d["beta"])
    return conv.to(device).requires_grad_(False), norm.to(device).requires_grad_(False)


@functools.lru_cache(maxsize=None)
def case(shape, bias=True):
    """The case's fp64 inputs, its fp64 and fp32 CPU literal results and its GPU modules and input — computed once, never modified."""
    d = K.dwconv_ln_inputs(*shape, bias=bias)
    ref64 = K.dwconv_ln_literal(**d)
    ref32 = K.dwconv_ln_literal(**K.cast(d, torch.float32))
    assert torch.isfinite(ref32).all()
    conv, norm = modules(d)
    return d, ref64, ref32, conv, norm, d["x"].float().to(DEV)


def run(x, conv, norm, **kw):
    with torch.no_grad():
        return Fn.dwconv7x7_ln_tokens(x, conv, norm, **kw)


@pytest.mark.parametrize("shape", list(K.DWCONV_LN_SHAPES.values()), ids=list(K.DWCONV_LN_SHAPES))
def test_against_fp64_literal(shape):
    d, ref64, ref32, conv, norm, x = case(shape)
    assert Fn.dwconv7x7_ln_tokens_ok(x, conv, norm)
    out = run(x, conv, norm)
    assert out.shape == x.shape and out.is_contiguous() and torch.isfinite(out).all()
    check_4x({"out": out}, {"out": ref32}, {"out": ref64}, f"dwconv7x7_ln {shape} ")
    B, h, w, C = shape
    tok = run(x.view(B, h * w, C), conv, norm, hw=(h, w))                    # the (B, h w, C) form: the same launch
    assert tok.shape == (B, h * w, C) and torch.equal(tok.view(B, h, w, C), out)


@pytest.mark.parametrize("shape", [(2, 9, 13, 100), (2, 4, 5, 1536)])
def test_without_conv_bias(shape):
    d, ref64, ref32, conv, norm, x = case(shape, bias=False)
    assert conv.bias is None
    check_4x({"out": run(x, conv, norm)}, {"out": ref32}, {"out": ref64}, f"dwconv7x7_ln {shape} bias=None ")


def test_frames_inside_a_larger_buffer_equal_their_contiguous_copy():
    shape = B, h, w, C = (2, 9, 13, 100)
    _, _, _, conv, norm, x = case(shape)
    buf = torch.full((B, h * w + 5, C), 7.0, device=DEV)
    buf[:, :h * w] = x.view(B, h * w, C)
    view = buf[:, :h * w]
    assert not view.is_contiguous() and view.stride(0) == (h * w + 5) * C
    assert torch.equal(run(view, conv, norm, hw=(h, w)).view(B, h, w, C), run(x, conv, norm))


def test_two_calls_give_the_same_bits():
    for shape in ((1, 4, 70, 192), (2, 4, 5, 1536)):
        _, _, _, conv, norm, x = case(shape)
        assert torch.equal(run(x, conv, norm), run(x, conv, norm))


@pytest.mark.parametrize("C", [100, 1536])
def test_a_frames_bits_do_not_depend_on_its_batch(C):
    h, w = 5, 11
    d = K.dwconv_ln_inputs(3, h, w, C, seed=5)
    conv, norm = modules(d)
    x = d["x"].float().to(DEV)
    whole = run(x, conv, norm)
    for b in range(3):
        assert torch.equal(run(x[b:b + 1], conv, norm), whole[b:b + 1])
    poisoned = x.clone()
    poisoned[1, 2, 3, 4] = float("nan")
    got = run(poisoned, conv, norm)
    assert torch.equal(got[0], whole[0]) and torch.equal(got[2], whole[2])
    assert torch.isnan(got[1, 2, 3]).all() and torch.equal(got[1, :, 7:], whole[1, :, 7:])     # and only the filter's reach in its frame


def test_every_output_element_is_written():
    for shape in ((2, 9, 13, 100), (1, 4, 70, 192), (2, 4, 5, 1536)):
        _, _, _, conv, norm, x = case(shape)
        want = run(x, conv, norm)
        out = torch.full_like(x, float("nan"))
        got = run(x, conv, norm, out=out)
        assert got.data_ptr() == out.data_ptr() and torch.equal(out, want)


def test_capture_and_replay():
    shape = (2, 4, 5, 1536)
    _, _, _, conv, norm, x = case(shape)
    want = run(x, conv, norm)
    out = torch.zeros_like(x)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(x, conv, norm, out=out)                                         # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    out.fill_(float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(x, conv, norm, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_grad_enabled_with_a_trainable_parameter_raises():
    d = K.dwconv_ln_inputs(1, 3, 5, 8)
    conv, norm = modules(d)
    norm.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="no backward for dwconv7x7_ln_tokens"):
        Fn.dwconv7x7_ln_tokens(d["x"].float().to(DEV), conv, norm)


def test_unserved_width_raises_instead_of_running_torch():
    d = K.dwconv_ln_inputs(1, 3, 5, 6)
    conv, norm = modules(d)
    with pytest.raises(RuntimeError, match="DVIS_STRICT"):
        run(d["x"].float().to(DEV), conv, norm)


def test_refusals_name_the_value_and_agree_with_supported():
    K.check_dwconv_ln_refusals(native.lib(), ctypes)
