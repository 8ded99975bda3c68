"""Backward of the token-major depthwise 3 x 3 convolution (+ bias, + GELU) of the ViT-Adapter extractors' ConvFFN
(csrc/dwconv_tokens_backward.hip, Fn.dwconv3x3_tokens_backward) against the fp64 CPU autograd of the reference's composition
(adapter.py:61-98: transposes, grouped Conv2d, GELU, concatenation).  The project's rule: the kernel may be 4 x as far from the
fp64 run as the fp32 CPU run is wherever a tensor has >= MIN_SAMPLES elements; smaller tensors take rtol 2e-3 / atol 5e-4."""
import ctypes

import pytest
import torch

from vit_adapter_train_cases import DWCONV_CASES, check_4x, dwconv_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gpu(case, gelu, grad_out=None):
    from dvis_plus_amd import functions as Fn
    b = case["bias"]
    go = case["grad_out"] if grad_out is None else grad_out
    gx, gw, gb = Fn.dwconv3x3_tokens_backward(case["x"].to(DEV), case["levels"], case["weight"].to(DEV),
                                              None if b is None else b.to(DEV), go.to(DEV), gelu=gelu)
    out = {"grad_x": gx, "grad_weight": gw}
    if b is not None:
        out["grad_bias"] = gb
    else:
        assert gb is None
    return out


@pytest.mark.parametrize("gelu", [True, False], ids=["gelu", "linear"])
@pytest.mark.parametrize("name", list(DWCONV_CASES))
def test_backward_vs_fp64_cpu_autograd_of_the_composition(name, gelu):
    case = dwconv_case(name, gelu)
    got = _gpu(case, gelu)
    want = {k: v for k, v in case["cpu64"].items() if k != "out"}
    assert set(got) == set(want) and all(got[k].shape == want[k].shape for k in want)
    check_4x(got, case["cpu32"], want, what=f"{name} gelu={gelu}: ")


@pytest.mark.parametrize("name", ["stack of (6, 10)", "more strips than the bounded grid", "C260 (crosses the 256-channel workgroup column)"])
def test_two_runs_give_the_same_bits(name):
    case = dwconv_case(name, True)
    a, b = _gpu(case, True), _gpu(case, True)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("gelu", [True, False], ids=["gelu", "linear"])
def test_zero_grad_out_gives_exactly_zero_gradients(gelu):
    case = dwconv_case("stack of (6, 10)", gelu)
    got = _gpu(case, gelu, grad_out=torch.zeros_like(case["grad_out"]))
    assert all(int(torch.count_nonzero(v)) == 0 for v in got.values())
    # zero in one channel only: that channel's gradients are exactly zero, the others are not
    go = case["grad_out"].clone()
    go[..., 5] = 0
    got = _gpu(case, gelu, grad_out=go)
    assert int(torch.count_nonzero(got["grad_x"][..., 5])) == 0 and int(torch.count_nonzero(got["grad_weight"][5])) == 0
    assert float(got["grad_bias"][5]) == 0.0 and int(torch.count_nonzero(got["grad_bias"])) == go.shape[-1] - 1


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_grad_out_comes_back_non_finite(bad):
    case = dwconv_case("stack of (6, 10)", True)
    go = case["grad_out"].clone()
    tok, ch = 12 * 20 + 3 * 10 + 4, 6             # level 1 (6 x 10), row 3, column 4
    go[0, tok, ch] = bad
    got = _gpu(case, True, grad_out=go)
    assert not torch.isfinite(got["grad_x"][0, tok, ch])
    assert not torch.isfinite(got["grad_bias"][ch]) and not torch.isfinite(got["grad_weight"][ch]).any()
    others = [c for c in range(go.shape[-1]) if c != ch]
    assert torch.isfinite(got["grad_x"][..., others]).all() and torch.isfinite(got["grad_weight"][others]).all()
    assert torch.isfinite(got["grad_bias"][others]).all()


def test_autograd_through_dwconv3x3_tokens_equals_the_explicit_backward():
    from dvis_plus_amd import functions as Fn
    for name, gelu in (("stack of (6, 10)", True), ("no bias", False)):
        case = dwconv_case(name, gelu)
        b = case["bias"]
        leaves = [case["x"].to(DEV).requires_grad_(), case["weight"].to(DEV).requires_grad_()] + \
            ([] if b is None else [b.to(DEV).requires_grad_()])
        with torch.no_grad():
            plain = Fn.dwconv3x3_tokens(leaves[0], case["levels"], leaves[1], None if b is None else leaves[2], gelu=gelu)
        out = Fn.dwconv3x3_tokens(leaves[0], case["levels"], leaves[1], None if b is None else leaves[2], gelu=gelu)
        assert out.requires_grad and torch.equal(out, plain), "under autograd the forward is the same kernel"
        assert float((out.detach().cpu().double() - case["cpu64"]["out"]).abs().max()) <= 1e-5
        grads = torch.autograd.grad(out, leaves, case["grad_out"].to(DEV))
        want = _gpu(case, gelu)
        assert torch.equal(grads[0], want["grad_x"]) and torch.equal(grads[1], want["grad_weight"])
        assert b is None or torch.equal(grads[2], want["grad_bias"])
    # only the weight needs a gradient: the input gets none
    x = case["x"].to(DEV)
    w = case["weight"].to(DEV).requires_grad_()
    Fn.dwconv3x3_tokens(x, case["levels"], w, None).sum().backward()
    assert w.grad is not None and x.grad is None


def test_the_c_abi_refuses_what_the_forward_refuses():
    from dvis_plus_amd import native
    lib = native.lib()
    B, h, w, C = 2, 3, 5, 8
    n = h * w * C
    assert lib.dvis_dwconv3x3_tokens_backward_ws_bytes(B, h, w, C) == 4 * (B * n + 3 * 10 * C)      # dz + 3 workgroups' partial rows (12 strips)
    assert lib.dvis_dwconv3x3_tokens_backward_ws_bytes(B, h, w, 6) == -1 and lib.dvis_dwconv3x3_tokens_backward_ws_bytes(B, 0, w, C) == -1
    # the partial rows are bounded: 100 x as many tokens add the dz buffer's bytes only
    big = lib.dvis_dwconv3x3_tokens_backward_ws_bytes(B, 100 * 24, 176, C) - 4 * B * 100 * 24 * 176 * C
    assert big == lib.dvis_dwconv3x3_tokens_backward_ws_bytes(B, 24, 176, C) - 4 * B * 24 * 176 * C == 4 * 512 * 10 * C
    t = lambda *s: torch.zeros(*s, device=DEV)
    x, go, gx, wt, bias, gw, gb = t(B, h * w + 2, C), t(B, h * w + 2, C), t(B, h * w + 2, C), t(C, 9), t(C), t(C, 9), t(C)
    ws = t(lib.dvis_dwconv3x3_tokens_backward_ws_bytes(B, h, w, C) // 4 + 4)
    p = lambda tensor, off=0: ctypes.c_void_p(tensor.data_ptr() + off)
    stream = native.stream_ptr(x.device)
    stride = (h * w + 2) * C

    def call(x_=p(x), go_=p(go), wt_=p(wt), b_=p(bias), stride_=stride, C_=C, gx_=p(gx), gw_=p(gw), gb_=p(gb), ws_=p(ws)):
        return lib.dvis_dwconv3x3_tokens_backward(x_, go_, wt_, b_, 1, stride_, B, h, w, C_, gx_, gw_, gb_, ws_, stream)
    assert call() == 0
    assert call(gb_=None, b_=None) == 0                                          # no bias: no grad_bias
    for what, kw in (("C % 4", dict(C_=6)), ("x alignment", dict(x_=p(x, 4))), ("grad_out alignment", dict(go_=p(go, 8))),
                     ("grad_x alignment", dict(gx_=p(gx, 4))), ("workspace alignment", dict(ws_=p(ws, 4))),
                     ("bias alignment", dict(b_=p(bias, 4))), ("batch stride % 4", dict(stride_=stride + 2)),
                     ("batch stride too small", dict(stride_=n - 4)), ("null x", dict(x_=None)), ("null grad_out", dict(go_=None)),
                     ("null weight", dict(wt_=None)), ("null grad_x", dict(gx_=None)), ("null grad_weight", dict(gw_=None)),
                     ("null workspace", dict(ws_=None)), ("grad_x aliases grad_out", dict(gx_=p(go))),
                     ("grad_x aliases x", dict(gx_=p(x)))):
        assert call(**kw) != 0, what
        assert b"dwconv3x3_tokens_backward" in lib.dvis_last_error(), what
    torch.cuda.synchronize()
    # the python wrapper's own refusals
    from dvis_plus_amd import functions as Fn
    with pytest.raises(RuntimeError, match="dwconv3x3_tokens_backward"):
        Fn.dwconv3x3_tokens_backward(t(1, 15, 6), [(3, 5)], t(6, 1, 3, 3), None, t(1, 15, 6))
    with pytest.raises(RuntimeError, match="grad_out"):
        Fn.dwconv3x3_tokens_backward(t(1, 15, 8), [(3, 5)], t(8, 1, 3, 3), None, t(1, 14, 8))
