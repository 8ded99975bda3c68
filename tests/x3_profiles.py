"""Operand profiles at the edges of the split-f16 ("x3") window, and the error model the kernels are held to.

A plain helper module (imported by tests/test_x3_error_model_cpu.py and tests/test_x3_operand_range_gpu.py).

The window (dvis_plus_amd/csrc/x3_common.h: split8, x3_pack_fragment; dvis_plus_amd/functions.py: _x3_exp)
-----------------------------------------------------------------------------------------------------------
An fp32 activation x is scaled by s = 2^xexp (exact) and cut into two f16 terms, both rounded to nearest even:

    hi = f16(x s),   lo = f16(x s - hi),   x s = hi + lo + r.

* f16 has an 11-bit significand (unit roundoff u = 2^-11): |x s - hi| <= u |x s|, and |r| <= u |lo| <= 2^-22 |x s| as long as
  `lo` is a normal f16 number.
* The largest finite f16 is 65504 and everything from 65520 on rounds to inf, so |x| < 65520 / 2^xexp is served and
  |x| = 65520 / 2^xexp is the first value refused (`limit`): hi = inf, lo = -inf, every product with them inf or NaN.
* Below |x s| = 2^-3 the low term (|lo| <= 2^-14) is an f16 subnormal, a multiple of 2^-24: then |r| <= 2^-25 in scaled units
  whatever x is (the same holds once hi itself is subnormal) — an absolute floor of 2^-(25 + xexp) per element.
* A weight matrix is scaled by 2^e with max|W| 2^e in [2^13, 2^14) and cut the same way.  Its elements below 2^-3 / 2^e carry
  the floor 2^-25 / 2^e, and 2^-e = max|W| / (max|W| 2^e) lies in (2^-14, 2^-13] max|W|.

The kernels issue three of the four products of (hi + lo)(hi + lo): hi hi + hi lo + lo hi (x3_common.h, mma_item: `wl xh`,
`wh xl`, `wh xh`), accumulated in fp32.  Per product x_k w_k, relative to |x_k| |w_k|: the two residuals r contribute at most
2^-22 each, the dropped lo lo product at most u^2 = 2^-22.  That is the first term of `bound`; the accumulation's own rounding
is not derived but MEASURED on the fp32 torch formulation of the same operands (`e_ref`, never on the kernel) and enters with
the factor 1.25 the existing tests already give it.  The two floors are the second and third term:

    |y - y64| <= (3 2^-22 + 1.25 e_ref) S + 2^-(25 + xexp) sum_k |W_nk| + 2^-(25 + e) sum_k |x_mk|,    S = |x| |W|^T + |b|.

Third term: 2^-(25 + e) lies in [2^-39, 2^-38) max|W|.  The lower end, 2^-39 max|W|, is the first guess one writes down; the
emulation in tests/test_x3_error_model_cpu.py refutes it (`edge_in` against `heavy_tail`: one activation of 4094.99 meets a weight
2^16 below the matrix maximum whose low term is subnormal, and that single product carries the row's error: 1.63 times the
2^-39 form).  The floor is a property of the exponent, so the model uses the exponent itself (`weight_exp`, the definition of
functions._x3_exp within the +-60 the pack kernels take).

`op`: every kernel of the family is a linear map of (x, W, b); `bound` takes that map as `op(x, W, b)` (default: x W^T + b) and
evaluates it on (|x|, |W|, |b|), (1, |W|, 0) and (|x|, 1, 0) — for a convolution the sums over k become sums over the receptive
field inside the image, which is what the floors are.

Through a LayerNorm (`ln_bound`)
--------------------------------
out_i = g_i n_i + beta_i with n = (v - mean(v)) / sigma, sigma^2 = var(v) + eps, over the C features of a row.  For a
perturbation d of v, to first order

    d n_i = (d_i - mean(d) - n_i mean(n d)) / sigma,

so with |d_i| <= B_i elementwise:  |d out_i| <= |g_i| / sigma (B_i + mean(B) + |n_i| mean(|n| B)).  All of it in fp64 from the
fp64 pre-norm row.  The issue's short form (B_i |g_i| / sigma) is the first of the three summands; the other two are the shift of
the row's mean and of its variance, which a row with one dominant element makes as large as the first.  The normalisation's own
fp32 rounding is again measured on torch's fp32 `layer_norm` of the rounded fp64 pre-norm rows and added as 1.25 e_ln.
"""
import math

import torch

F16_OVERFLOW = 65520.0          # the smallest magnitude that rounds to inf in f16 (halfway between 65504 and 2^16, tie to even)


def limit(xexp):
    """The smallest |x| the kernels refuse at activation exponent `xexp`: 4095 at 4, 16380 at 2."""
    return F16_OVERFLOW / 2.0 ** xexp


def below_limit(xexp):
    """The largest fp32 value that must still be served."""
    return float(torch.nextafter(torch.tensor(limit(xexp), dtype=torch.float32), torch.tensor(0.0)))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def edge_rows(M):
    """Rows of the `edge_in` plants: first, middle (the `edge_out` / NaN row), last."""
    return sorted({0, M // 2, M - 1})


def plants(name, shape, seed):
    """[(row, column, kind)] of the planted elements of `edge_in`, `edge_out` and `nonfinite`."""
    M, K = shape
    g = _gen(seed + 7919)
    cols = torch.randint(0, K, (3,), generator=g).tolist()
    if name == "edge_in":
        return [(r, cols[i], "below") for i, r in enumerate(edge_rows(M))]
    if name == "edge_out":
        return [(M // 2, cols[1], "limit")]
    if name == "nonfinite":
        # (a single row holds both, in different columns)
        return [(M // 2, cols[1], "nan"), (M - 1, cols[2], "inf") if M > 1 else (0, (cols[1] + 1) % K, "inf")]
    return []


ACTIVATIONS = ("edge_in", "edge_out", "dominated", "log_uniform", "floor", "nonfinite", "normal")
IN_WINDOW = ("edge_in", "dominated", "log_uniform", "floor")


def profile(name, shape, xexp, seed):
    """(M, K) fp32 CPU activations of profile `name` for a kernel whose split exponent is `xexp`."""
    M, K = shape
    g = _gen(seed)
    x = torch.randn(M, K, generator=g)
    if name == "normal":
        return x
    if name in ("edge_in", "edge_out", "nonfinite"):
        sign = 1.0
        for r, c, kind in plants(name, shape, seed):
            x[r, c] = {"below": sign * below_limit(xexp), "limit": limit(xexp), "nan": float("nan"), "inf": float("inf")}[kind]
            sign = -sign
        return x
    if name == "dominated":
        x = x * 2.0 ** -6
        pos = torch.randint(0, K, (M,), generator=g)
        big = (1e3 + 2e3 * torch.rand(M, generator=g)) * (torch.randint(0, 2, (M,), generator=g) * 2 - 1)
        x[torch.arange(M), pos] = big
        return x
    if name == "log_uniform":
        u = torch.rand(M, K, generator=g, dtype=torch.float64) * (11 - xexp + 4 + 20) - 20
        return (torch.exp2(u) * (torch.randint(0, 2, (M, K), generator=g) * 2 - 1)).float()
    if name == "floor":
        return x * torch.exp2(-(torch.arange(M) % 25).float())[:, None]
    raise KeyError(name)


WEIGHTS = ("xavier", "heavy_tail", "pow2_max", "zero_row", "zero", "subnormal_max", "tiny_max", "nan")
POW2_K = (-3, 0, 5)


def zero_row_index(N):
    return N // 3


def nan_index(N, K):
    return N // 2, K // 3


def weights(name, N, K, seed, k=0):
    """(N, K) fp32 CPU weight matrix of profile `name` (`k`: the exponent of `pow2_max`)."""
    g = _gen(seed)
    a = math.sqrt(6.0 / (N + K))
    w = (torch.rand(N, K, generator=g) * 2 - 1) * a
    if name == "xavier":
        return w
    if name == "heavy_tail":
        w = w * torch.exp(torch.randn(N, K, generator=g) * 2.0)
        w.view(-1)[int(torch.randint(0, N * K, (1,), generator=g))] = 1e3 * float(w.abs().max())
        return w
    if name == "pow2_max":
        m = float(w.abs().max())
        if m >= 2.0 ** k:
            w = w * (0.99 * 2.0 ** k / m)
        w.view(-1)[int(w.abs().argmax())] = 2.0 ** k
        return w
    if name == "zero_row":
        w[zero_row_index(N)] = 0.0
        return w
    if name == "zero":
        return torch.zeros(N, K)
    if name == "subnormal_max":
        return (w.double() / float(w.abs().max()) * 1e-39).float()
    if name == "tiny_max":
        # max|w| = 2^-70: the pack exponent is held at 60, max|w| 2^60 = 2^-10 — hi keeps its 11 bits, the low terms are subnormal
        return (w.double() / float(w.abs().max()) * 2.0 ** -70).float()
    if name == "nan":
        w[nan_index(N, K)] = float("nan")
        return w
    raise KeyError(name)


def bias(N, seed):
    return torch.randn(N, generator=_gen(seed + 104729))


def weight_exp(W):
    """e with max|W| 2^e in [2^13, 2^14), within +-60; 0 for a zero matrix."""
    m = float(W.abs().max())
    return 0 if m == 0.0 or m != m else max(-60, min(60, 14 - math.frexp(m)[1]))


def linear_op(x, W, b):
    y = x @ W.t()
    return y if b is None else y + b


def bound(x, W, b, xexp, e_ref, op=linear_op, gain=1.0, acc_steps=0):
    """Elementwise fp64 bound on |y_kernel - y64| for y = op(x, W, b) (see the module docstring).  `gain`: the Lipschitz
    constant of an activation applied to y inside the kernel (1 for ReLU), applied to the split's terms.  `acc_steps`: where the
    measured e_ref cannot stand for the kernel's accumulation (a deep contraction: the library sums in blocks, the kernels chain
    K / 16 matrix products into one fp32 accumulator), the chain's own worst case, 2^-24 S per step, is added."""
    x, W = x.double(), W.double()
    zb = None if b is None else torch.zeros_like(b, dtype=torch.float64)
    S = op(x.abs(), W.abs(), None if b is None else b.double().abs())
    floor_x = op(torch.ones_like(x), W.abs(), zb) * 2.0 ** -(25 + xexp)
    floor_w = op(x.abs(), torch.ones_like(W), zb) * 2.0 ** -(25 + weight_exp(W))
    return gain * (3 * 2.0 ** -22 * S + floor_x + floor_w) + (1.25 * e_ref + acc_steps * 2.0 ** -24) * S, S


def ln_bound(pre64, B, gamma, eps, e_ln):
    """Push the elementwise bound B on the pre-norm rows `pre64` through LayerNorm(gamma, beta, eps) — module docstring."""
    mean = pre64.mean(-1, keepdim=True)
    sigma = (pre64.var(-1, unbiased=False, keepdim=True) + eps).sqrt()
    n = (pre64 - mean) / sigma
    spread = B + B.mean(-1, keepdim=True) + n.abs() * (n.abs() * B).mean(-1, keepdim=True)
    return gamma.double().abs() / sigma * spread + 1.25 * e_ln


def split_f16(v64, exp):
    """(hi, lo) f16 terms of the fp32 values held in the fp64 tensor `v64`, scaled by 2^exp — the arithmetic of split8 /
    x3_pack_fragment: the scaling is exact (a power of two), the residual is formed in fp32."""
    s = torch.ldexp(v64, torch.tensor(exp))              # exact; may exceed the fp32 range for a subnormal weight
    hi = s.half()
    lo = (s - hi.double()).float().half()
    return hi, lo


def emulate(x, W, b, xexp, wexp, products=("hh", "hl", "lh"), lo_sign=1.0):
    """x W^T + b as the kernels form it, with the f16 products accumulated in fp64: what a correct implementation computes
    before its own accumulation rounding.  `products` / `lo_sign`: the mutations the CPU test must catch."""
    xh, xl = split_f16(x.double(), xexp)
    wh, wl = split_f16(W.double(), wexp)
    xh, xl, wh, wl = xh.double(), lo_sign * xl.double(), wh.double(), lo_sign * wl.double()
    acc = torch.zeros(x.shape[0], W.shape[0], dtype=torch.float64)
    if "hh" in products:
        acc += xh @ wh.t()
    if "hl" in products:
        acc += xh @ wl.t()
    if "lh" in products:
        acc += xl @ wh.t()
    y = torch.ldexp(acc, torch.tensor(-(xexp + wexp)))
    return y if b is None else y + b.double()
