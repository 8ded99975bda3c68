"""csrc/attention_backward.hip: the gradients of softmax(q k^T / sqrt(d)) v, their determinism, and the autograd wiring of
functions.attention.

Yardstick: tests/attention_backward_cases.py — per tensor 4 x the error of the worse of two fp32 CPU formulations against fp64 autograd
of the ``cpu_ops.attention`` composition on the same inputs, never the kernel's own output.  Every compared tensor has at least 64
elements except in the one-key case, which is exact.

With q = 0 every probability is exactly 1 / Lk; at Lk = 16 and integer v / grad_out every product and sum is exact in fp32, so dv
must be bit-equal to the fp64 result and dk must be zero whatever the order: indexing and chunk-edge errors show without a
tolerance.

The lattice walks the launch geometry (64 / 128 / 256 threads = 4 / 8 / 16 reduction lanes per query row, asserted through
functions.attention_backward_threads) and the 16-query chunk edge at both head dims.  One-hot attention (inputs of
tests/test_attention_edges_gpu.py: a target key per query that leads its row by >= 200 log2 units) makes dq and dk exactly zero and
dv an exact integer sum; rows whose maxima run from -900 to +900 log2 units need the max subtraction in front of the exponential.
Both assert their precondition on the CPU before the GPU is touched."""
import pytest
import torch

from attention_backward_cases import check_against_fp64, cpu_grads, draw
from test_attention_edges_gpu import assert_score_range, one_hot_inputs, one_hot_margin, score_range_inputs

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
    return draw(Lq, Lk, B, heads, d, seed, masked=False)[:4]


@pytest.mark.parametrize("Lq,Lk,B,heads,d", SHAPES)
def test_backward_against_fp64_and_determinism(Fn, Lq, Lk, B, heads, d):
    q, k, v, go = _draw(Lq, Lk, B, heads, d, 21)
    got, _ = check_against_fp64(Fn.attention_backward, q, k, v, go, heads, label=f"shape {(Lq, Lk, B, heads, d)}",
                                zero_error_takes_largest=False)
    again = Fn.attention_backward(*(t.cuda() for t in (q, k, v, go)), heads)
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
    ref = cpu_grads(q, k, v, go, heads, torch.float64)
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


# Lk -> threads of the launch (one per key, rounded up to 64 / 128 / 256; R = threads / 16 lanes reduce a query row): the switches at
# 64 / 65 and 128 / 129, Lk below R (2, 3: reduction lanes that own no key), Lk around the 16-key granule of nothing in particular
# (15 / 16 / 17 — the kernel has no key tile, so these must not matter), the limit 256.
LATTICE_LK = {2: 64, 3: 64, 15: 64, 16: 64, 17: 64, 63: 64, 64: 64, 65: 128, 127: 128, 128: 128, 129: 256, 255: 256, 256: 256}
LATTICE_LQ = [1, 15, 16, 17, 33]          # the 16-query chunk: below, at, one past, two chunks + 1


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("Lk", sorted(LATTICE_LK))
def test_backward_lattice_of_thread_counts_and_chunk_edges(Fn, Lk, d):
    """B = 2, heads = 2: every compared tensor has at least 128 elements.

    Lq = 1 is the sharpest row of the lattice: dv = p x grad_out of a single query averages nothing, so the rounding of the scores
    shows undiluted.  With q . k as ONE fma chain over the head dim the kernel missed the bound here (Lk 17, d 64, dv: 4.759e-07
    against an fp32 CPU figure of 1.145e-07, ratio 4.16); the kernel now sums four chains pairwise (2.394e-07, ratio 2.09)."""
    assert Fn.attention_backward_threads(Lk) == LATTICE_LK[Lk]
    B, heads = 2, 2
    for Lq in LATTICE_LQ:
        q, k, v, go = _draw(Lq, Lk, B, heads, d, 31 + Lq)
        check_against_fp64(Fn.attention_backward, q, k, v, go, heads, label=f"lattice {(Lq, Lk, B, heads, d)}")


@pytest.mark.parametrize("Lq,Lk,d", [(33, 256, 64), (100, 100, 32)])
def test_one_hot_attention_gradients_are_exact(Fn, Lq, Lk, d):
    """Every probability is exactly 0 or 1: dS = P o (dP - D) is exactly 0, so dq == dk == 0, and dv[t] is the integer sum of the
    grad_out rows whose query chose t (several queries share a key, most keys are chosen by none)."""
    B, heads = 2, 2
    q, k, v, pi = one_hot_inputs(Lq, Lk, d, 41 + Lq, integer_v=True)
    go = torch.randint(-3, 4, (Lq, B, heads * d), generator=torch.Generator().manual_seed(42)).float()
    assert one_hot_margin(q, k, d, pi) >= 200.0
    want_dv = torch.zeros(Lk, B, heads * d)
    for b in range(B):
        want_dv[:, b].index_add_(0, pi[b], go[:, b])
    assert any(pi[b].unique().numel() < Lq for b in range(B))
    cq, ck, cv = cpu_grads(q, k, v, go, heads, torch.float32)
    assert (cq == 0).all() and (ck == 0).all() and torch.equal(cv, want_dv)       # the reference alone meets the claim
    dq, dk, dv = (t.cpu() for t in Fn.attention_backward(q.cuda(), k.cuda(), v.cuda(), go.cuda(), heads))
    assert (dq == 0).all() and (dk == 0).all()
    assert torch.equal(dv, want_dv)


# one case per launch geometry
RANGE_SHAPES = [(20, 40, 32), (33, 100, 32), (17, 256, 64)]


@pytest.mark.parametrize("Lq,Lk,d", RANGE_SHAPES)
def test_backward_with_row_maxima_from_minus_900_to_plus_900_log2_units(Fn, Lq, Lk, d):
    """Without the subtraction of the row maximum 2^s overflows for the rows near +900 and underflows to l = 0 for those near -900.
    Bound: the file's measured 4 x e32 per tensor; a tensor whose fp32 CPU error is 0 because its exact gradient is 0 would take the
    largest fp32 CPU error among the three tensors as its baseline (the per-parameter check of tests/test_refiner_train_gpu.py sets
    the precedent)."""
    heads = 2
    q, k, v = score_range_inputs(Lq, Lk, d, 51 + Lk)
    go = torch.randn(q.shape, generator=torch.Generator().manual_seed(52))
    assert_score_range(q, k, d)
    check_against_fp64(Fn.attention_backward, q, k, v, go, heads, label=f"score range {(Lq, Lk, d)}")


def test_autograd_over_the_score_range(Fn):
    Lq, Lk, d = RANGE_SHAPES[1]
    heads = 2
    q, k, v = (t.cuda() for t in score_range_inputs(Lq, Lk, d, 53))
    go = torch.randn(q.shape, generator=torch.Generator().manual_seed(54)).cuda()
    assert_score_range(q.cpu(), k.cpu(), d)
    with torch.no_grad():
        plain = Fn.attention(q, k, v, heads)
    assert torch.isfinite(plain).all()
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    out = Fn.attention(*leaves, heads)
    assert out.requires_grad and torch.equal(out.detach(), plain)
    grads = torch.autograd.grad(out, leaves, go)
    want = Fn.attention_backward(q, k, v, go, heads)
    assert all(torch.equal(g, w) for g, w in zip(grads, want))
