"""The split-f16 error model (tests/x3_profiles.py) against an emulation of the arithmetic in torch on the CPU: the operand
profiles of tests/test_x3_operand_range_gpu.py are chosen so that a CORRECT three-product implementation stays inside the bound
— shown here without a GPU — and an implementation with a wrong low term or a missing cross product does not."""
import math

import pytest
import torch

import x3_profiles as P
from dvis_plus_amd import functions as Fn

# the shapes the GPU tests run the linear kernels at (one ragged row tile; K = 256 is 16 k-steps)
M, K, N = 129, 256, 288
WEIGHT_CASES = [("xavier", 0), ("heavy_tail", 0), ("pow2_max", -3), ("pow2_max", 0), ("pow2_max", 5), ("zero_row", 0), ("zero", 0),
                ("subnormal_max", 0), ("tiny_max", 0)]
PAIRS = [(a, w, k) for a in P.IN_WINDOW for (w, k) in WEIGHT_CASES[:2]] + [("normal", w, k) for (w, k) in WEIGHT_CASES[2:]]


def _operands(act, wname, k, xexp):
    return P.profile(act, (M, K), xexp, 11), P.weights(wname, N, K, 12, k=k), P.bias(N, 13)


def _worst(y, x, W, b, xexp):
    B, S = P.bound(x, W, b, xexp, 0.0)
    ref = x.double() @ W.double().t() + b.double()
    return float(((y - ref).abs() / B).max()), float(((y - ref).abs() / S).max())


@pytest.mark.parametrize("xexp", [Fn.X3_XEXP, Fn.X3_CONV_XEXP])
@pytest.mark.parametrize("act,wname,k", PAIRS)
def test_a_correct_split_stays_inside_the_bound(act, wname, k, xexp):
    x, W, b = _operands(act, wname, k, xexp)
    for wexp in {Fn._x3_exp(W), Fn._x3_wexp(W)}:       # the exponent of the definition, and the one handed to the pack kernels
        ratio, rel = _worst(P.emulate(x, W, b, xexp, wexp), x, W, b, xexp)
        print(f"emulation {act:>11} x {wname}{k if wname == 'pow2_max' else ''} xexp {xexp} wexp {wexp}: err/bound {ratio:.3f}  err/S {rel:.2e}")
        assert ratio <= 1.0


@pytest.mark.parametrize("mutation", [dict(lo_sign=-1.0), dict(products=("hh", "hl")), dict(products=("hh", "lh"))])
def test_a_wrong_low_term_or_a_missing_cross_product_leaves_the_bound(mutation):
    for act in ("dominated", "log_uniform"):
        x, W, b = _operands(act, "xavier", 0, Fn.X3_XEXP)
        ratio, _ = _worst(P.emulate(x, W, b, Fn.X3_XEXP, Fn._x3_exp(W), **mutation), x, W, b, Fn.X3_XEXP)
        assert ratio > 1.0, (act, mutation, ratio)


@pytest.mark.parametrize("xexp", [Fn.X3_XEXP, Fn.X3_CONV_XEXP])
def test_the_limit_is_65520_over_the_scale(xexp):
    assert P.limit(xexp) == {4: 4095.0, 2: 16380.0}.get(xexp, P.limit(xexp))
    x = P.profile("edge_in", (M, K), xexp, 11)
    assert float(x.abs().max()) == P.below_limit(xexp) < P.limit(xexp)
    hi, lo = P.split_f16(x.double(), xexp)
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    x = P.profile("edge_out", (M, K), xexp, 11)
    hi, _ = P.split_f16(x.double(), xexp)
    bad = ~torch.isfinite(hi)
    assert int(bad.sum()) == 1 and bool(bad[M // 2].any())


@pytest.mark.parametrize("wname,k", WEIGHT_CASES)
def test_weight_exponent_fills_the_f16_range(wname, k):
    W = P.weights(wname, N, K, 12, k=k)
    m = float(W.abs().max())
    e = Fn._x3_exp(W)
    if m == 0.0:
        assert e == 0
        return
    assert 2.0 ** 13 <= math.ldexp(m, e) < 2.0 ** 14, (m, e)
    # what the pack kernels get is a float scale 2^wexp and the kernels a float 2^-(xexp + wexp): both must be normal floats
    we = Fn._x3_wexp(W)
    assert abs(we) <= 60 and (we == e or abs(e) > 60)


def test_nan_and_inf_maxima_have_an_exponent():
    assert Fn._x3_exp(P.weights("nan", N, K, 12)) == 0
    W = P.weights("xavier", N, K, 12)
    W[3, 4] = float("inf")
    assert abs(Fn._x3_wexp(W)) <= 60
