"""csrc/window_attention.hip against the fp64 CPU run of cpu_ops.window_attention, by the project's rule (at most 4 x as far from
fp64 as the fp32 CPU run is), and its determinism / isolation / coverage properties."""
import pytest
import torch

import swin_cases as S
from dvis_plus_amd import functions as Fn
from vit_adapter_train_cases import check_4x

pytestmark = pytest.mark.gpu
DEV = "cuda"


def run(case, **over):
    c = dict(case, **over)
    gpu = lambda t: None if t is None else t.to(DEV)
    with torch.no_grad():
        return Fn.window_attention(gpu(c["qkv"]), gpu(c["qkv_bias"]), gpu(c["table"]), *c["args"])


@pytest.mark.parametrize("shifted", [False, True], ids=["shift0", "shifted"])
@pytest.mark.parametrize("name", list(S.KERNEL_CASES))
def test_kernel_vs_fp64(name, shifted):
    case = S.kernel_case(name, shifted)
    out = run(case)
    assert torch.isfinite(out).all()
    check_4x({"out": out}, case["cpu32"], case["cpu64"], f"{name} shift {case['args'][-1]}: ")


@pytest.mark.parametrize("shifted", [False, True], ids=["shift0", "shifted"])
def test_no_qkv_bias(shifted):
    name = "pads on both axes"
    case = S.kernel_case(name, shifted, bias=False)
    assert case["qkv_bias"] is None
    check_4x({"out": run(case)}, case["cpu32"], case["cpu64"], f"{name}, qkv_bias=None: ")


@pytest.mark.parametrize("name", ["pads on both axes", "map shorter than a window"])
def test_large_scores_need_the_row_maximum(name):
    """A table of +-30 and q, k scaled x 8: exp() of a raw score overflows, the row maximum has to be subtracted."""
    case = S.kernel_case(name, True, table_scale=30.0, qk_scale=8.0)
    out = run(case)
    assert torch.isfinite(out).all()
    check_4x({"out": out}, case["cpu32"], case["cpu64"], f"{name}, large scores: ")


def test_same_bits_every_call_and_for_every_batch_size():
    case = S.kernel_case("more work units than a bounded grid would hold", True)
    B, H, W, heads, ws, shift = case["args"]
    assert B == 3
    a, b = run(case), run(case)
    assert torch.equal(a, b)
    alone = run(case, qkv=case["qkv"][1:2], args=(1, H, W, heads, ws, shift))
    assert torch.equal(alone[0], a[1])


def test_a_nan_stays_in_its_frame():
    case = S.kernel_case("pads on both axes", True)
    qkv = case["qkv"].clone()
    qkv[0, 17] = float("nan")
    out = run(case, qkv=qkv)
    assert torch.isnan(out[0]).any() and torch.isfinite(out[1]).all()
    assert torch.equal(out[1], run(case)[1])


@pytest.mark.parametrize("name", ["pads on both axes", "map shorter than a window"])
def test_every_unpadded_row_is_written(name):
    """The output buffer is pre-filled with a sentinel: no element keeps it, and the rows equal a run into a fresh buffer."""
    case = S.kernel_case(name, True)
    B, H, W, heads, ws, shift = case["args"]
    SENTINEL = -12345.0
    buf = torch.full((B, H * W, heads * 32), SENTINEL, device=DEV)
    with torch.no_grad():
        got = Fn.window_attention(case["qkv"].to(DEV), case["qkv_bias"].to(DEV), case["table"].to(DEV), *case["args"], out=buf)
    assert got is buf and not (buf == SENTINEL).any() and torch.equal(buf, run(case))


def test_input_that_requires_grad_raises():
    case = S.kernel_case("one window, tile tails", False)
    qkv = case["qkv"].to(DEV).requires_grad_()
    with pytest.raises(RuntimeError, match="no window-attention backward"):
        Fn.window_attention(qkv, case["qkv_bias"].to(DEV), case["table"].to(DEV), *case["args"])


def test_unsupported_window_raises_under_the_strict_default(monkeypatch):
    monkeypatch.delenv("DVIS_STRICT", raising=False)
    qkv, bias, table = (t.to(DEV) for t in S.attention_inputs(1, 9, 9, 2, 3, d=8))
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"ws=3 with head dim d=8"):
        Fn.window_attention(qkv, bias, table, 1, 9, 9, 2, 3, 1)
