"""csrc/msda_backward.hip, msda_fused_bwd_kernel: the backward of the fused MSDeformAttn forward from the forward's own inputs (raw
offset / logit rows, reference points), through Fn.msda_fused_backward and the autograd Function behind Fn.msda_fused.

Reference rule: the fp64 CPU autograd of the torch formulation (softmax, locations, grid_sample) on the same fp32-valued inputs;
the fp32 CPU run of the same formulation is the baseline, and the kernel may be 4 x as far from the fp64 run as that (the project's
bound) wherever a tensor has >= MIN_SAMPLES elements.  The small lattice cases use rtol = 2e-3, atol = 5e-4 — the fp32 rule of
test_msda_gpu.py::test_forward_backward_vs_oracle — at O(1) inputs.  Sampling coordinates are kept >= 1e-3 pixel from the integers
(where the bilinear gradient jumps) by construction, asserted on the CPU before the GPU is touched."""
import ctypes

import pytest
import torch

from segmenter_train_cases import (MIN_SAMPLES, coordinate_margin, fused_torch_grads, make_fused_inputs, pixel_coordinates)

pytestmark = pytest.mark.gpu
DEV = "cuda"
LATTICE = dict(rtol=2e-3, atol=5e-4)
NAMES = ("grad_value", "grad_offsets", "grad_logits")


def _fn():
    from dvis_plus_amd import functions as Fn
    return Fn


def _gpu(inputs):
    return [t.to(DEV) for t in inputs]


def _backward(inputs, L, P=4, deterministic=False):
    value, s, lsi, ref, off, lg, go = _gpu(inputs)
    return _fn().msda_fused_backward(value, s, lsi, ref, off, lg, go, L, P, deterministic=deterministic)


def _reference(inputs, L, P, dtype):
    value, s, lsi, ref, off, lg, go = inputs
    return fused_torch_grads(value, s, ref, off, lg, go, L, P, dtype)[1:]


MAIN = {"r50_like": (3, 8, 32, [(5, 8), (10, 16), (20, 32)], None),
        "four_levels": (2, 8, 32, [(4, 5), (8, 10), (16, 20), (32, 40)], 130),
        "one_level_d64": (2, 16, 64, [(20, 32)], 777)}


@pytest.mark.parametrize("case", list(MAIN), ids=list(MAIN))
@pytest.mark.parametrize("deterministic", [False, True], ids=["atomics", "fixed_point"])
def test_main_shapes_within_four_times_the_fp32_cpu_error(case, deterministic):
    N, M, D, shapes, Lq = MAIN[case]
    inputs = make_fused_inputs(N, M, D, shapes, Lq, seed=N * 13 + D)
    L = len(shapes)
    ref64 = _reference(inputs, L, 4, torch.float64)
    ref32 = _reference(inputs, L, 4, torch.float32)
    got = _backward(inputs, L, deterministic=deterministic)
    for name, g, r64, r32 in zip(NAMES, got, ref64, ref32):
        assert g.shape == r64.shape and r64.numel() >= MIN_SAMPLES
        err = (g.cpu().double() - r64).abs().max().item()
        base = (r32.double() - r64).abs().max().item()
        print(f"{case} {name}: err {err:.3e}, fp32 CPU {base:.3e}, ratio {err / base:.2f}")
        assert err <= 4 * base, (name, err, base)


@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("L", [1, 3, 4])
def test_lattice_of_small_shapes(D, L):
    """Ragged groups per block (Lq * M * N pairs against 8 or 4 groups per block) and both group widths; Nref in {1, N}."""
    shapes = [(6, 9), (3, 5), (4, 4), (2, 3)][:L]
    M = 2
    for Lq in (1, 7, 8, 9, 63, 65):
        for N, nref in ((1, 1), (2, 1), (2, 2)):
            inputs = make_fused_inputs(N, M, D, shapes, Lq, seed=Lq * 7 + N + nref, nref=nref)
            want = _reference(inputs, L, 4, torch.float64)
            got = _backward(inputs, L)
            for name, g, w in zip(NAMES, got, want):
                torch.testing.assert_close(g.cpu().double(), w, **LATTICE, msg=lambda m: f"Lq {Lq} N {N} Nref {nref} {name}: {m}")


def test_strided_rows_equal_contiguous_copies():
    """Offsets and logits sliced out of ONE (N * Lq, 3 M L P) projection, as the module's fused projection hands them over."""
    N, M, D, shapes, Lq = 2, 8, 32, [(5, 8), (10, 16), (20, 32)], 77
    value, s, lsi, ref, off, lg, go = make_fused_inputs(N, M, D, shapes, Lq, seed=5)
    proj = torch.cat([off, lg], 1).to(DEV)
    wo = off.shape[1]
    v, s_, lsi_, ref_, go_ = _gpu((value, s, lsi, ref, go))
    Fn = _fn()
    a = Fn.msda_fused_backward(v, s_, lsi_, ref_, proj[:, :wo], proj[:, wo:], go_, 3, 4, deterministic=True)
    b = Fn.msda_fused_backward(v, s_, lsi_, ref_, proj[:, :wo].contiguous(), proj[:, wo:].contiguous(), go_, 3, 4, deterministic=True)
    assert not proj[:, wo:].is_contiguous()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_samples_outside_the_maps_give_exact_zeros():
    """Every sample more than one pixel outside its map: no corner is read, all three gradients are exactly zero."""
    N, M, D, shapes, Lq = 2, 2, 32, [(5, 8), (3, 4), (6, 6)], 19
    value, s, lsi, ref, off, lg, go = make_fused_inputs(N, M, D, shapes, Lq, seed=9)
    off = off.view(N, Lq, M, 3, 4, 2).clone()
    far = torch.tensor([[-12.5, 3.0], [3.0, -9.5], [14.5, 2.0], [2.0, 11.5]])      # left, above, right, below: > 1 pixel out everywhere
    off[:] = far[None, None, None, None, :, :]
    c = pixel_coordinates(off, ref, s)
    W, H = s[:, 1].view(1, 1, 1, 3, 1), s[:, 0].view(1, 1, 1, 3, 1)
    outside = (c[..., 0] < -1.001) | (c[..., 0] > W + 0.001) | (c[..., 1] < -1.001) | (c[..., 1] > H + 0.001)
    assert bool(outside.all())
    for det in (False, True):
        for g in _backward((value, s, lsi, ref, off.reshape(N * Lq, -1), lg, go), 3, deterministic=det):
            assert bool((g == 0).all())


def test_samples_on_the_border_rows_and_columns():
    """Coordinates in (-1, 0) and (size - 1, size): one or two of the four corners lie outside the map."""
    N, M, D, shapes, Lq = 1, 2, 64, [(5, 8), (3, 4), (6, 6)], 40
    value, s, lsi, ref, off, lg, go = make_fused_inputs(N, M, D, shapes, Lq, seed=11)
    g = torch.Generator().manual_seed(12)
    ref = torch.full_like(ref, 0.5)
    off = off.view(N, Lq, M, 3, 4, 2).clone()
    for l, (h, w) in enumerate(shapes):
        frac = 0.05 + 0.9 * torch.rand(N, Lq, M, 4, 2, generator=g)                  # distance into the border band
        lo = torch.rand(N, Lq, M, 4, 2, generator=g) < 0.5
        size = torch.tensor([w, h], dtype=torch.float32)
        target = torch.where(lo, -frac, size - 1 + frac)                             # pixel coordinate in (-1, 0) or (size - 1, size)
        off[:, :, :, l] = target + 0.5 - 0.5 * size                                  # coordinate = ref * size + off - 0.5
    c = pixel_coordinates(off, ref, s)
    size = torch.stack([s[:, 1], s[:, 0]], -1).view(1, 1, 1, 3, 1, 2)
    assert bool((((c > -1) & (c < 0)) | ((c > size - 1) & (c < size))).all()) and float(coordinate_margin(off, ref, s)) >= 1e-3
    inputs = (value, s, lsi, ref, off.reshape(N * Lq, -1), lg, go)
    want = _reference(inputs, 3, 4, torch.float64)
    assert float(want[1].abs().max()) > 0
    for name, got, w in zip(NAMES, _backward(inputs, 3), want):
        torch.testing.assert_close(got.cpu().double(), w, **LATTICE, msg=lambda m: f"{name}: {m}")


def test_equal_logits():
    """a = 1 / (L P) everywhere: the logit gradients of a (n, q, m) row cancel, and grad_value is the unfused deterministic
    backward's on the same locations and that weight."""
    N, M, D, shapes, Lq = 2, 2, 32, [(5, 8), (10, 16), (20, 32)], 150
    value, s, lsi, ref, off, lg, go = make_fused_inputs(N, M, D, shapes, Lq, seed=21)
    lg = torch.zeros_like(lg)
    gv, _, gl = _backward((value, s, lsi, ref, off, lg, go), 3, deterministic=True)
    rows = gl.cpu().double().view(N * Lq * M, 12)
    assert bool((rows.sum(1).abs() <= 1e-6 * rows.abs().sum(1)).all()), float((rows.sum(1).abs() / rows.abs().sum(1)).max())
    Fn = _fn()
    v, s_, lsi_, ref_, off_, go_ = _gpu((value, s, lsi, ref, off, go))
    norm = torch.stack([s_[:, 1], s_[:, 0]], -1).float()[None, None, None, :, None, :]
    loc = (ref_[:, :, None, :, None, :] + off_.view(N, Lq, M, 3, 4, 2) / norm).contiguous()
    w = torch.full((N, Lq, M, 3, 4), 1.0 / 12, device=DEV)
    want = Fn.ms_deform_attn_backward(v, s_, lsi_, loc, w, go_, deterministic=True)[0]
    torch.testing.assert_close(gv, want, **LATTICE)


def test_one_logit_far_above_the_rest():
    N, M, D, shapes, Lq = 1, 2, 32, [(5, 8), (10, 16), (20, 32)], 50
    value, s, lsi, ref, off, lg, go = make_fused_inputs(N, M, D, shapes, Lq, seed=23)
    lg = torch.zeros_like(lg).view(N * Lq, M, 12)
    lg[:, :, 5] = 80.0
    got = _backward((value, s, lsi, ref, off, lg.view(N * Lq, -1), go), 3)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    gl = got[2].cpu().view(N * Lq, M, 12)
    others = torch.cat([gl[:, :, :5], gl[:, :, 6:]], -1)
    assert float(others.abs().max()) <= 1e-30


def _colliding_inputs():
    """Half of the queries sample ONE cell per level (thousands of colliding atomics) and one grad_out row is 1e4 x the rest."""
    N, M, D, shapes, Lq = 2, 8, 32, [(5, 8), (10, 16), (20, 32)], 400
    value, s, lsi, ref, off, lg, go = make_fused_inputs(N, M, D, shapes, Lq, seed=31)
    ref[:, :Lq // 2] = 0.37
    off = off.view(N, Lq, M * 24).clone()
    off[:, :Lq // 2] = 0
    go[0, 0] *= 1e4
    assert float(coordinate_margin(off.view(N, Lq, M, 3, 4, 2), ref, s)) >= 1e-3
    return (value, s, lsi, ref, off.view(N * Lq, -1), lg, go)


def test_determinism():
    inputs = _colliding_inputs()
    a = _backward(inputs, 3, deterministic=True)
    b = _backward(inputs, 3, deterministic=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    d = _backward(inputs, 3, deterministic=False)
    assert torch.equal(a[1], d[1]) and torch.equal(a[2], d[2])
    torch.testing.assert_close(a[0], d[0], rtol=1e-4, atol=1e-5 * float(a[0].abs().max()))
    # torch's switch selects the fixed-point form through autograd
    Fn = _fn()
    value, s, lsi, ref, off, lg, go = _gpu(inputs)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        v, o, l_ = (t.clone().requires_grad_() for t in (value, off, lg))
        out = Fn.msda_fused(v, s, lsi, ref, o, l_, 3, 4)
        out.backward(go.view_as(out))
        assert torch.equal(v.grad, a[0]) and torch.equal(o.grad, a[1]) and torch.equal(l_.grad, a[2])
    finally:
        torch.use_deterministic_algorithms(prev)


def test_non_finite_grad_out_comes_back_non_finite():
    """The fixed-point form has no image of a NaN / Inf: EVERY grad_value element comes back NaN.  Float atomics can only reach the
    cells the bad grad_out element is added to (as dvis_msda_backward): every one of THOSE is non-finite — they are the cells a
    grad_out that is 1 in that element and 0 elsewhere gives a non-zero gradient.  Finite input stays finite."""
    inputs = list(make_fused_inputs(1, 8, 32, [(6, 10), (12, 20), (3, 5)], 300, seed=3))
    for det in (False, True):
        assert bool(torch.isfinite(_backward(inputs, 3, deterministic=det)[0]).all())
    one = torch.zeros_like(inputs[6])
    one[0, 7, 3] = 1.0
    touched = _backward(inputs[:6] + [one], 3, deterministic=False)[0] != 0
    assert int(touched.sum()) > 0
    for bad in (float("nan"), float("inf")):
        go = inputs[6].clone()
        go[0, 7, 3] = bad
        gv = _backward(inputs[:6] + [go], 3, deterministic=True)[0]
        assert not bool(torch.isfinite(gv).any()), f"grad_out with {bad}: finite grad_value from the fixed-point form"
        gv = _backward(inputs[:6] + [go], 3, deterministic=False)[0]
        assert not bool(torch.isfinite(gv[touched]).any()), f"grad_out with {bad}: a touched cell of the float-atomic form is finite"


def test_non_finite_logits_come_back_non_finite_from_the_fixed_point_form():
    """A NaN or +Inf logit makes the pair's weights NaN; a NaN contribution has no fixed-point image, so the kernel reports it and
    grad_value comes back NaN, as the unfused deterministic form's weight maximum would make it.  A -Inf logit is a weight of 0."""
    inputs = list(make_fused_inputs(1, 8, 32, [(6, 10), (12, 20), (3, 5)], 300, seed=4))
    for bad in (float("nan"), float("inf")):
        lg = inputs[5].clone()
        lg[11, 17] = bad
        gv, _, gl = _backward(inputs[:5] + [lg, inputs[6]], 3, deterministic=True)
        assert not bool(torch.isfinite(gv).any()) and not bool(torch.isfinite(gl[11, 12:24]).any())
    lg = inputs[5].clone()
    lg[11, 17] = float("-inf")
    assert all(bool(torch.isfinite(g).all()) for g in _backward(inputs[:5] + [lg, inputs[6]], 3, deterministic=True))


def _c_abi(value, s, lsi, ref, off, lg, go, L, P):
    """The C entry point, called directly (float atomics form) -> return code."""
    from dvis_plus_amd import native
    N, S, M, D = value.shape
    Lq = ref.shape[1]
    gv = torch.zeros(N, S, M, D, device=DEV)
    goff = torch.zeros(N * Lq, M * L * P * 2, device=DEV)
    gl = torch.zeros(N * Lq, M * L * P, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    keep = go.contiguous()
    rc = native.lib().dvis_msda_fused_backward(p(value), p(s), p(lsi), p(ref), ref.shape[0], p(off), off.stride(0), p(lg), lg.stride(0),
                                               p(keep), N, S, M, D, L, Lq, P, p(gv), p(goff), p(gl), None, native.stream_ptr(value.device))
    torch.cuda.synchronize()
    if rc != 0:
        assert not bool(gv.any()) and not bool(goff.any()) and not bool(gl.any())      # nothing was launched
    return rc


def test_refusals():
    Fn = _fn()
    shapes = [(5, 8), (3, 4)]
    # D = 30
    value, s, lsi, ref, off, lg, go = _gpu(make_fused_inputs(1, 2, 30, shapes[:1], 9, seed=1))
    with pytest.raises(RuntimeError, match="unsupported"):
        Fn.msda_fused_backward(value, s, lsi, ref, off, lg, go, 1, 4)
    assert _c_abi(value, s, lsi, ref, off, lg, go, 1, 4) != 0
    # (L, P) = (2, 3)
    value, s, lsi, ref, off, lg, go = _gpu(make_fused_inputs(1, 2, 32, shapes, 9, P=3, seed=2))
    with pytest.raises(RuntimeError, match="unsupported"):
        Fn.msda_fused_backward(value, s, lsi, ref, off, lg, go, 2, 3)
    assert _c_abi(value, s, lsi, ref, off, lg, go, 2, 3) != 0
    # misaligned rows: the offsets start 4 bytes into a 16-byte aligned buffer
    value, s, lsi, ref, off, lg, go = _gpu(make_fused_inputs(1, 2, 32, shapes[:1], 9, seed=3))
    buf = torch.zeros(off.shape[0], off.shape[1] + 4, device=DEV)
    shifted = buf[:, 1:1 + off.shape[1]]
    shifted.copy_(off)
    assert shifted.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="aligned"):
        Fn.msda_fused_backward(value, s, lsi, ref, shifted, lg, go, 1, 4)
    assert _c_abi(value, s, lsi, ref, shifted, lg, go, 1, 4) != 0
    # a row stride that is no multiple of 4 floats
    odd = torch.zeros(off.shape[0], off.shape[1] + 1, device=DEV)[:, :off.shape[1]]
    with pytest.raises(RuntimeError, match="aligned"):
        Fn.msda_fused_backward(value, s, lsi, ref, odd, lg, go, 1, 4)
    assert _c_abi(value, s, lsi, ref, odd, lg, go, 1, 4) != 0
    # reference points that require grad: the kernel has no gradient for them
    r = ref.clone().requires_grad_()
    with pytest.raises(RuntimeError, match="reference"):
        Fn.msda_fused_backward(value, s, lsi, r, off, lg, go, 1, 4)
    with pytest.raises(RuntimeError, match="reference"):
        Fn.msda_fused(value.clone().requires_grad_(), s, lsi, r, off, lg, 1, 4)
    # and the accepted call goes through
    assert _c_abi(value, s, lsi, ref, off, lg, go, 1, 4) == 0


def test_autograd_function():
    """Fn.msda_fused: the forward is msda_fused_forward's bits, with and without a requires-grad input; its backward through
    autograd is msda_fused_backward, also into the ONE projection the two row views are sliced from."""
    Fn = _fn()
    N, M, D, shapes, Lq = 2, 8, 32, [(5, 8), (10, 16), (20, 32)], None
    value, s, lsi, ref, off, lg, go = _gpu(make_fused_inputs(N, M, D, shapes, Lq, seed=41, nref=1))
    want = Fn.msda_fused_forward(value, s, lsi, ref, off, lg, 3, 4, shapes_host=shapes)
    assert torch.equal(Fn.msda_fused(value, s, lsi, ref, off, lg, 3, 4, shapes_host=shapes), want)
    wo = off.shape[1]
    v = value.clone().requires_grad_()
    proj = torch.cat([off, lg], 1).requires_grad_()
    out = Fn.msda_fused(v, s, lsi, ref, proj[:, :wo], proj[:, wo:], 3, 4, shapes_host=shapes)
    assert out.requires_grad and torch.equal(out, want)
    out.backward(go)
    gv, goff, gl = Fn.msda_fused_backward(value, s, lsi, ref, off, lg, go, 3, 4, deterministic=True)
    assert torch.equal(proj.grad[:, :wo], goff) and torch.equal(proj.grad[:, wo:], gl)
    torch.testing.assert_close(v.grad, gv, rtol=1e-4, atol=1e-5)
    with torch.no_grad():
        assert torch.equal(Fn.msda_fused(v, s, lsi, ref, off, lg, 3, 4), want)
