"""csrc/attention_backward.hip: the gradients of softmax(q k^T / sqrt(d)) v, their determinism, and the autograd wiring of
functions.attention.

Yardstick: fp64 autograd of the ``cpu_ops.attention`` composition on the CPU.  The bound of each of dq, dk, dv is measured, not
chosen: 4 x the error of an fp32 CPU run against that fp64 run on the same inputs (4 = the project's factor for a different
summation order, tests/test_mask_gemm_backward_gpu.py).  The kernel's exponential is the hardware's base-2 instruction where the
CPU's is expf, so the fp32 CPU figure is the worse of two formulations per tensor: torch's softmax, and the same composition
with torch.exp2 on scores scaled by scale * log2(e).  It is never the kernel's own output.  Every compared tensor has at least
64 elements (test_tracker_train_gpu.cpu_baselines says why) except in the one-key case, which is exact.

With q = 0 every probability is exactly 1 / Lk; at Lk = 16 and integer v / grad_out every product and sum is exact in fp32, so dv
must be bit-equal to the fp64 result and dk must be zero whatever the order: indexing and chunk-edge errors show without a
tolerance."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (Lq, Lk, B, heads, d)
SHAPES = [
    (5, 5, 8, 2, 32),          # the fixture's time attention, below one 16-row chunk
    (21, 21, 100, 8, 32),      # production time attention
    (100, 100, 3, 8, 32),      # object attention; 100 is no multiple of 16
    (200, 200, 2, 8, 32),      # 200 queries: several query chunks, 256 threads
    (8, 24, 2, 2, 32),         # Lq != Lk
    (17, 256, 1, 2, 64),       # B = 1 stride case, d = 64, the Lk limit
]


@pytest.fixture(scope="module")
def Fn():
    from dvis_plus_amd import functions
    return functions


def _draw(Lq, Lk, B, heads, d, seed):
    gen = torch.Generator().manual_seed(seed)
    C = heads * d
    return (torch.randn(Lq, B, C, generator=gen), torch.randn(Lk, B, C, generator=gen), torch.randn(Lk, B, C, generator=gen),
            torch.randn(Lq, B, C, generator=gen))


def _cpu_grads(q, k, v, go, heads, dtype, base2=False):
    """(dq, dk, dv) by torch autograd of the cpu_ops.attention composition in `dtype`; base2: the softmax as exp2 on scores scaled
    by scale * log2(e), normalised by their sum (what the kernel computes)."""
    from dvis_plus_amd import cpu_ops
    q, k, v = (t.to(dtype).clone().requires_grad_() for t in (q, k, v))
    if not base2:
        out = cpu_ops.attention(q, k, v, heads)
    else:
        Lq, B, C = q.shape
        Lk, d = k.shape[0], C // heads
        split = lambda t, n: t.reshape(n, B, heads, d).permute(1, 2, 0, 3)
        s = (split(q, Lq) @ split(k, Lk).transpose(-1, -2)) * ((1.0 / d ** 0.5) * math.log2(math.e))
        e = torch.exp2(s - s.amax(-1, keepdim=True))
        out = ((e / e.sum(-1, keepdim=True)) @ split(v, Lk)).permute(2, 0, 1, 3).reshape(Lq, B, C)
    return torch.autograd.grad(out, (q, k, v), go.to(dtype))


def _bounds(q, k, v, go, heads):
    ref = _cpu_grads(q, k, v, go, heads, torch.float64)
    a = _cpu_grads(q, k, v, go, heads, torch.float32)
    b = _cpu_grads(q, k, v, go, heads, torch.float32, base2=True)
    base = [max((x.double() - r).abs().max().item(), (y.double() - r).abs().max().item()) for x, y, r in zip(a, b, ref)]
    return ref, base


@pytest.mark.parametrize("Lq,Lk,B,heads,d", SHAPES)
def test_backward_against_fp64_and_determinism(Fn, Lq, Lk, B, heads, d):
    q, k, v, go = _draw(Lq, Lk, B, heads, d, 21)
    ref, base = _bounds(q, k, v, go, heads)
    dev = [t.cuda() for t in (q, k, v, go)]
    got = Fn.attention_backward(*dev, heads)
    for name, x, r, b in zip(("dq", "dk", "dv"), got, ref, base):
        assert x.shape == r.shape and x.dtype == torch.float32 and x.is_contiguous() and r.numel() >= 64
        err = (x.cpu().double() - r).abs().max().item()
        print(f"shape {(Lq, Lk, B, heads, d)} {name}: err {err:.3e} fp32 CPU err {b:.3e} ratio {err / b:.2f}")
    for x, r, b in zip(got, ref, base):
        assert (x.cpu().double() - r).abs().max().item() <= 4 * b
    again = Fn.attention_backward(*dev, heads)
    assert all(torch.equal(x, y) for x, y in zip(got, again))


def test_one_key_is_exact(Fn):
    Lq, Lk, B, heads, d = 1, 1, 2, 2, 32
    q, k, v, go = (t.cuda() for t in _draw(Lq, Lk, B, heads, d, 22))
    dq, dk, dv = Fn.attention_backward(q, k, v, go, heads)
    assert (dq == 0).all() and (dk == 0).all()
    assert torch.equal(dv, go)


@pytest.mark.parametrize("Lq", [16, 100, 200])
def test_uniform_probabilities_are_exact(Fn, Lq):
    Lk, B, heads, d = 16, 3, 2, 32
    gen = torch.Generator().manual_seed(23)
    C = heads * d
    q = torch.zeros(Lq, B, C)
    k = torch.randn(Lk, B, C, generator=gen)
    v = torch.randint(-3, 4, (Lk, B, C), generator=gen).float()
    go = torch.randint(-3, 4, (Lq, B, C), generator=gen).float()
    ref = _cpu_grads(q, k, v, go, heads, torch.float64)
    dq, dk, dv = Fn.attention_backward(q.cuda(), k.cuda(), v.cuda(), go.cuda(), heads)
    assert torch.equal(dv.cpu(), ref[2].float())
    assert (dk == 0).all()
    assert ref[1].abs().max().item() == 0
    assert torch.isfinite(dq).all()


def test_views_are_bit_equal_to_contiguous_copies(Fn):
    heads, d = 2, 32
    C = heads * d
    gen = torch.Generator().manual_seed(24)
    # slices of one fused in-projection
    L, B = 24, 3
    qkv = torch.randn(L, B, 3 * C, generator=gen).cuda()
    go = torch.randn(L, B, C, generator=gen).cuda()
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    want = Fn.attention_backward(q.contiguous(), k.contiguous(), v.contiguous(), go, heads)
    got = Fn.attention_backward(q, k, v, go, heads)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    leaf = qkv.clone().requires_grad_()
    out = Fn.attention(leaf[..., :C], leaf[..., C:2 * C], leaf[..., 2 * C:], heads)
    (g_leaf,) = torch.autograd.grad(out, leaf, go)
    assert torch.equal(g_leaf, torch.cat(want, dim=-1))
    # the per-frame view of TemporalRefiner._attention: (T, clips * Q, C) memory read as (Q, T * clips, C)
    T, clips, Q = 5, 2, 8
    per_frame = lambda z: z.view(T * clips, Q, C).transpose(0, 1)
    bufs = [torch.randn(T, clips * Q, C, generator=gen).cuda() for _ in range(4)]
    views = [per_frame(z) for z in bufs]
    assert not views[0].is_contiguous()
    want = Fn.attention_backward(*(z.contiguous() for z in views), heads)
    got = Fn.attention_backward(*views, heads)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    # a non-contiguous grad_out alone
    got = Fn.attention_backward(*(z.contiguous() for z in views[:3]), views[3], heads)
    assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_a_batch_entry_does_not_depend_on_its_batch(Fn):
    Lq, Lk, B, heads, d = 40, 100, 8, 2, 32
    q, k, v, go = (t.cuda() for t in _draw(Lq, Lk, B, heads, d, 25))
    full = Fn.attention_backward(q, k, v, go, heads)
    alone = Fn.attention_backward(*(t[:, :1].contiguous() for t in (q, k, v, go)), heads)
    assert all(torch.equal(x[:, 0], y[:, 0]) for x, y in zip(full, alone))
    sliced = Fn.attention_backward(*(t[:, :1] for t in (q, k, v, go)), heads)     # B = 1 views with the batch's row stride
    assert all(torch.equal(x, y) for x, y in zip(sliced, alone))


@pytest.mark.parametrize("needs", [(True, True, True), (True, False, False), (False, True, True)])
def test_autograd_wiring(Fn, needs):
    Lq, Lk, B, heads, d = 21, 21, 4, 2, 32
    q, k, v, go = (t.cuda() for t in _draw(Lq, Lk, B, heads, d, 26))
    with torch.no_grad():
        plain = Fn.attention(q, k, v, heads)
    assert torch.equal(Fn.attention(q, k, v, heads), plain)
    leaves = [t.clone().requires_grad_(n) for t, n in zip((q, k, v), needs)]
    out = Fn.attention(*leaves, heads)
    assert out.requires_grad and torch.equal(out.detach(), plain)
    want = Fn.attention_backward(q, k, v, go, heads)
    wanted = [t for t, n in zip(leaves, needs) if n]
    grads = torch.autograd.grad(out, wanted, go)
    assert all(torch.equal(g, w) for g, w in zip(grads, [w for w, n in zip(want, needs) if n]))
    with torch.no_grad():                                             # grad mode off: the call it always was, out= included
        buf = torch.empty_like(plain)
        assert Fn.attention(*leaves, heads, out=buf) is buf and torch.equal(buf, plain)


def test_backward_copies_a_gradient_that_misses_the_view_contract(Fn):
    """The upstream gradient of a concatenation on the last dim is a narrowed view one float past a 16-byte boundary."""
    Lq, Lk, B, heads, d = 8, 24, 2, 2, 32
    q, k, v, go = (t.cuda() for t in _draw(Lq, Lk, B, heads, d, 27))
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    out = torch.cat([torch.zeros(Lq, B, 1, device="cuda"), Fn.attention(*leaves, heads)], dim=-1)
    wide = torch.cat([torch.zeros(Lq, B, 1, device="cuda"), go], dim=-1)
    grads = torch.autograd.grad(out, leaves, wide)
    want = Fn.attention_backward(q, k, v, go, heads)
    assert all(torch.equal(g, w) for g, w in zip(grads, want))


def test_refusals_are_host_side(Fn):
    heads, d = 2, 32
    C = heads * d
    z = lambda L, c=C, **kw: torch.zeros(L, 2, c, device="cuda", **kw)
    q = z(4).requires_grad_()
    with pytest.raises(RuntimeError, match="mask"):
        Fn.attention(q, z(4), z(4), heads, mask=torch.zeros(2, 4, 4, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="out="):
        Fn.attention(q, z(4), z(4), heads, out=z(4))
    with pytest.raises(RuntimeError, match="256"):
        Fn.attention_backward(z(4), z(257), z(257), z(4), heads)
    with pytest.raises(RuntimeError, match="256"):
        Fn.attention(q, z(257), z(257), heads)
    with pytest.raises(RuntimeError, match="32 or 64"):
        Fn.attention_backward(z(4, 32), z(4, 32), z(4, 32), z(4, 32), 2)
    with pytest.raises(RuntimeError, match="float32"):
        Fn.attention_backward(z(4), z(4), z(4, dtype=torch.float64), z(4), heads)
    with pytest.raises(RuntimeError, match="inner stride"):
        Fn.attention_backward(z(4, 2 * C)[..., ::2], z(4), z(4), z(4), heads)
