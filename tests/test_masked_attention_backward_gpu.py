"""csrc/masked_attention_backward.hip: the gradients of softmax(q k^T / sqrt(d), blocked keys left out) v over long key sequences,
their determinism, the mask semantics of the forward kernel, and the autograd wiring of functions.masked_attention.

Yardstick: tests/attention_backward_cases.py with the mask applied in all three CPU runs — per tensor 4 x the error of the worse of two
fp32 CPU formulations against fp64 autograd of ``cpu_ops.attention(..., mask, allowed_count)``; a tensor whose fp32 CPU error is 0
takes the largest of the three.  It is never the kernel's own output.  Every compared tensor has at least 64 elements.

The lattice takes its key and query tiles from functions.masked_attention_backward_plan, the function the launch consults.  The
exact cases (uniform probabilities over exactly 16 open keys; one-hot attention with the inputs of
tests/test_attention_edges_gpu.py) first assert that the fp32 CPU reference alone meets their claim."""
import pytest
import torch

from attention_backward_cases import check_against_fp64, cpu_grads, cuda, draw
from test_attention_edges_gpu import assert_score_range, one_hot_inputs, one_hot_margin, score_range_inputs

pytestmark = pytest.mark.gpu

# (Lq, Lk, B, heads, d, masked)
SHAPES = [
    (6, 18, 4, 2, 32, True),           # g17's levels: 18 ...
    (6, 288, 4, 2, 32, True),          # ... and 288 keys (two key tiles)
    (100, 35, 2, 8, 32, True),         # Lk odd: the mask's rows are not 4-byte aligned
    (100, 920, 2, 8, 32, True),
    (200, 1440, 1, 8, 32, True),
    (17, 300, 1, 2, 64, True),
    (100, 300, 2, 8, 32, False),
]


@pytest.fixture(scope="module")
def Fn():
    from dvis_plus_amd import functions
    return functions


@pytest.mark.parametrize("Lq,Lk,B,heads,d,masked", SHAPES)
def test_backward_against_fp64_and_determinism(Fn, Lq, Lk, B, heads, d, masked):
    q, k, v, go, mask, allowed = draw(Lq, Lk, B, heads, d, 61, masked)
    if masked:
        assert Lk < 64 or 0.2 < (mask == 0).float().mean().item() < 0.3
    got, _ = check_against_fp64(Fn.masked_attention_backward, q, k, v, go, heads, mask, allowed, f"shape {(Lq, Lk, B, heads, d, masked)}")
    again = Fn.masked_attention_backward(*cuda(q, k, v, go), heads, *cuda(mask, allowed))
    assert all(torch.equal(x, y) for x, y in zip(got, again))


def test_plan_is_the_launch_geometry(Fn):
    p = Fn.masked_attention_backward_plan(100, 5760, 32)
    assert p.threads == p.key_tile and p.n_key_tiles == -(-5760 // p.key_tile) and 1 <= p.query_tile <= 256
    assert p.lds_bytes <= 160 * 1024 and Fn.masked_attention_backward_plan(256, 65536, 64).lds_bytes <= 160 * 1024
    assert Fn.masked_attention_backward_plan(1, 1, 64).n_key_tiles == 1
    for bad in ((257, 10, 32), (10, 65537, 32), (10, 10, 16), (0, 10, 32)):
        with pytest.raises(RuntimeError):
            Fn.masked_attention_backward_plan(*bad)


LATTICE_LK = {"1": lambda kt: 1, "2": lambda kt: 2, "3": lambda kt: 3, "kt-1": lambda kt: kt - 1, "kt": lambda kt: kt,
              "kt+1": lambda kt: kt + 1, "2kt+1": lambda kt: 2 * kt + 1, "257": lambda kt: 257}


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("which", sorted(LATTICE_LK))
def test_backward_lattice_of_key_tiles_and_query_chunks(Fn, which, d):
    """Lk in {1, 2, 3, kt - 1, kt, kt + 1, 2 kt + 1, 257} x Lq in {1, qt - 1, qt, qt + 1, 100} (Lq = 256 once, at Lk = kt) with the
    key tile kt and the query chunk qt of the plan.  B = 2, heads = 2: every compared tensor has at least 128 elements.  Half of the
    keys are open, so at Lk = 1 .. 3 some rows are blocked everywhere (count 0: they ignore their mask)."""
    p = Fn.masked_attention_backward_plan(100, 300, d)
    kt, qt = p.key_tile, p.query_tile
    Lk = LATTICE_LK[which](kt)
    B, heads = 2, 2
    for Lq in [1, qt - 1, qt, qt + 1, 100] + ([256] if which == "kt" else []):
        plan = Fn.masked_attention_backward_plan(Lq, Lk, d)
        assert (plan.key_tile, plan.query_tile) == (kt, qt) and plan.n_key_tiles == -(-Lk // kt)
        q, k, v, go, mask, allowed = draw(Lq, Lk, B, heads, d, 71 + Lq, open_fraction=0.5)
        check_against_fp64(Fn.masked_attention_backward, q, k, v, go, heads, mask, allowed, f"lattice {(Lq, Lk, B, heads, d)}")


@pytest.mark.parametrize("Lq", [10, 17])
def test_uniform_probabilities_over_16_open_keys_are_exact(Fn, Lq):
    """q = 0: every open key of a row has probability exactly 1 / 16 — the row's maximum and sum are kept as two numbers, and the 16
    keys of a row are spread over both key tiles —, integer v / grad_out make every product and sum exact in fp32."""
    Lk, B, heads, d = 300, 2, 2, 32
    gen = torch.Generator().manual_seed(81)
    C = heads * d
    q = torch.zeros(Lq, B, C)
    k = torch.randn(Lk, B, C, generator=gen)
    v = torch.randint(-3, 4, (Lk, B, C), generator=gen).float()
    go = torch.randint(-3, 4, (Lq, B, C), generator=gen).float()
    mask = torch.ones(B, Lq, Lk, dtype=torch.uint8)
    for b in range(B):
        for i in range(Lq):
            mask[b, i, torch.randperm(Lk, generator=gen)[:16]] = 0
    allowed = (mask == 0).sum(-1).to(torch.int32)
    assert (allowed == 16).all() and not torch.equal(mask[0, 0], mask[0, 1])
    never = (mask == 1).all(1).T                                                   # (Lk, B): blocked for every query
    assert never.any() and (mask[:, :, :256] == 0).any() and (mask[:, :, 256:] == 0).any()
    ref = cpu_grads(q, k, v, go, heads, torch.float64, mask, allowed)
    c32 = cpu_grads(q, k, v, go, heads, torch.float32, mask, allowed)
    assert torch.equal(c32[2], ref[2].float()) and (c32[1] == 0).all() and ref[1].abs().max().item() == 0
    dq, dk, dv = (t.cpu() for t in Fn.masked_attention_backward(*cuda(q, k, v, go), heads, *cuda(mask, allowed)))
    assert torch.equal(dv, ref[2].float())
    assert (dk == 0).all()
    assert (dv[never] == 0).all() and (dk[never] == 0).all()
    assert torch.isfinite(dq).all()


@pytest.mark.parametrize("Lq,Lk,d", [(33, 300, 64), (100, 600, 32)])
def test_one_hot_attention_gradients_are_exact(Fn, Lq, Lk, d):
    """Every probability is exactly 0 or 1: dS is exactly 0, so dq == dk == 0, and dv[t] is the integer sum of the grad_out rows whose
    query chose t.  The target key stays open, the others are blocked at random."""
    B, heads = 2, 2
    q, k, v, pi = one_hot_inputs(Lq, Lk, d, 91 + Lq, integer_v=True)
    gen = torch.Generator().manual_seed(92)
    go = torch.randint(-3, 4, (Lq, B, heads * d), generator=gen).float()
    assert one_hot_margin(q, k, d, pi) >= 200.0
    mask = torch.rand(B, Lq, Lk, generator=gen) < 0.7
    mask.scatter_(-1, pi[..., None], False)
    mask = mask.to(torch.uint8)
    allowed = (mask == 0).sum(-1).to(torch.int32)
    want_dv = torch.zeros(Lk, B, heads * d)
    for b in range(B):
        want_dv[:, b].index_add_(0, pi[b], go[:, b])
    cq, ck, cv = cpu_grads(q, k, v, go, heads, torch.float32, mask, allowed)
    assert (cq == 0).all() and (ck == 0).all() and torch.equal(cv, want_dv)       # the reference alone meets the claim
    dq, dk, dv = (t.cpu() for t in Fn.masked_attention_backward(*cuda(q, k, v, go), heads, *cuda(mask, allowed)))
    assert (dq == 0).all() and (dk == 0).all()
    assert torch.equal(dv, want_dv)


def test_a_row_with_count_zero_ignores_its_mask(Fn):
    Lq, Lk, B, heads, d = 20, 300, 2, 2, 32
    q, k, v, go, _, _ = draw(Lq, Lk, B, heads, d, 101, masked=False)
    mask = torch.zeros(B, Lq, Lk, dtype=torch.uint8)
    mask[1, 7] = 1
    allowed = (mask == 0).sum(-1).to(torch.int32)
    assert allowed[1, 7] == 0 and (allowed > 0).sum() == B * Lq - 1
    dev = cuda(q, k, v, go)
    dmask, dallowed = cuda(mask, allowed)
    plain = Fn.masked_attention_backward(*dev, heads)
    got = Fn.masked_attention_backward(*dev, heads, dmask, dallowed)
    assert torch.equal(got[0][7, 1], plain[0][7, 1])
    assert all(torch.equal(x, y) for x, y in zip(got, plain))


def test_blocking_a_key_removes_its_contribution_from_the_row(Fn):
    Lq, Lk, B, heads, d = 5, 300, 2, 2, 32
    q, k, v, go, mask, allowed = draw(Lq, Lk, B, heads, d, 111)
    b0, r0, j = 1, 3, 277                      # key j of batch entry b0: open for row r0 alone
    mask[b0, :, j] = 1
    mask[b0, r0, j] = 0
    allowed = (mask == 0).sum(-1).to(torch.int32)
    before, _ = check_against_fp64(Fn.masked_attention_backward, q, k, v, go, heads, mask, allowed, "one open row")
    assert before[1][j, b0].abs().max() > 0 and before[2][j, b0].abs().max() > 0
    mask[b0, r0, j] = 1
    allowed = (mask == 0).sum(-1).to(torch.int32)
    after, ref = check_against_fp64(Fn.masked_attention_backward, q, k, v, go, heads, mask, allowed, "blocked for every row")
    assert ref[1][j, b0].abs().max() == 0 and ref[2][j, b0].abs().max() == 0
    assert (after[1][j, b0] == 0).all() and (after[2][j, b0] == 0).all()
    assert torch.equal(after[2][:, 0], before[2][:, 0])                            # the other batch entry: untouched


# one tile / two tiles / d = 64 with a partial second tile
RANGE_SHAPES = [(33, 100, 32), (20, 300, 32), (17, 257, 64)]


@pytest.mark.parametrize("Lq,Lk,d", RANGE_SHAPES)
def test_backward_with_row_maxima_from_minus_900_to_plus_900_log2_units(Fn, Lq, Lk, d):
    heads = 2
    q, k, v = score_range_inputs(Lq, Lk, d, 121 + Lk)
    go = torch.randn(q.shape, generator=torch.Generator().manual_seed(122))
    assert_score_range(q, k, d)
    mask = torch.rand(2, Lq, Lk, generator=torch.Generator().manual_seed(Lk)) < 0.5
    mask[:, :, 0] = False
    assert_score_range(q, k, d, mask)
    mask = mask.to(torch.uint8)
    allowed = (mask == 0).sum(-1).to(torch.int32)
    check_against_fp64(Fn.masked_attention_backward, q, k, v, go, heads, mask, allowed, f"score range {(Lq, Lk, d)}")


def test_views_are_bit_equal_to_contiguous_copies(Fn):
    heads, d = 2, 32
    C = heads * d
    gen = torch.Generator().manual_seed(131)
    Lq, Lk, B = 24, 300, 3
    qbuf = torch.randn(Lq, B, 3 * C, generator=gen).cuda()
    kvbuf = torch.randn(Lk, B, 3 * C, generator=gen).cuda()
    go = torch.randn(Lq, B, C, generator=gen).cuda()
    mask = (torch.rand(B, Lq, Lk, generator=gen) >= 0.25).to(torch.uint8).cuda()
    allowed = (mask == 0).sum(-1).to(torch.int32)
    q, k, v = qbuf[..., :C], kvbuf[..., C:2 * C], kvbuf[..., 2 * C:]
    assert not q.is_contiguous() and not k.is_contiguous()
    want = Fn.masked_attention_backward(q.contiguous(), k.contiguous(), v.contiguous(), go, heads, mask, allowed)
    got = Fn.masked_attention_backward(q, k, v, go, heads, mask, allowed)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    # a non-contiguous grad_out: (B, Lq, C) memory read as (Lq, B, C)
    go_t = go.transpose(0, 1).contiguous().transpose(0, 1)
    assert not go_t.is_contiguous() and torch.equal(go_t, go)
    got = Fn.masked_attention_backward(q.contiguous(), k.contiguous(), v.contiguous(), go_t, heads, mask, allowed)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    # a B = 1 slice with the batch's row stride
    one = lambda t: t[:, 1:2]
    alone = Fn.masked_attention_backward(*(one(t).contiguous() for t in (q, k, v, go)), heads, mask[1:2].contiguous(),
                                         allowed[1:2].contiguous())
    sliced = Fn.masked_attention_backward(one(q), one(k), one(v), one(go), heads, mask[1:2].contiguous(), allowed[1:2].contiguous())
    assert all(torch.equal(x, y) for x, y in zip(sliced, alone))
    assert all(torch.equal(x[:, 0], y[:, 1]) for x, y in zip(alone, want))


def test_a_batch_entry_does_not_depend_on_its_batch(Fn):
    Lq, Lk, B, heads, d = 40, 600, 8, 2, 32
    q, k, v, go, mask, allowed = cuda(*draw(Lq, Lk, B, heads, d, 141))
    full = Fn.masked_attention_backward(q, k, v, go, heads, mask, allowed)
    for b in (0, 5):
        alone = Fn.masked_attention_backward(*(t[:, b:b + 1].contiguous() for t in (q, k, v, go)), heads, mask[b:b + 1].contiguous(),
                                             allowed[b:b + 1].contiguous())
        assert all(torch.equal(x[:, b], y[:, 0]) for x, y in zip(full, alone))


@pytest.mark.parametrize("needs", [(True, True, True), (True, False, False), (False, True, True), (False, False, True)])
@pytest.mark.parametrize("masked", [True, False])
def test_autograd_wiring(Fn, needs, masked):
    Lq, Lk, B, heads, d = 21, 300, 3, 2, 32
    q, k, v, go, mask, allowed = cuda(*draw(Lq, Lk, B, heads, d, 151, masked))
    with torch.no_grad():
        plain = Fn.attention(q, k, v, heads, mask, allowed)
        assert torch.equal(Fn.masked_attention(q, k, v, heads, mask, allowed), plain)
    assert torch.equal(Fn.masked_attention(q, k, v, heads, mask, allowed), plain)
    leaves = [t.clone().requires_grad_(n) for t, n in zip((q, k, v), needs)]
    out = Fn.masked_attention(*leaves, heads, mask, allowed)
    assert out.requires_grad and torch.equal(out.detach(), plain)
    want = Fn.masked_attention_backward(q, k, v, go, heads, mask, allowed)
    grads = torch.autograd.grad(out, [t for t, n in zip(leaves, needs) if n], go)
    assert all(torch.equal(g, w) for g, w in zip(grads, [w for w, n in zip(want, needs) if n]))
    with_out = Fn.masked_attention_backward(q, k, v, go, heads, mask, allowed, out=plain)
    assert all(torch.equal(x, y) for x, y in zip(with_out, want))


def test_backward_copies_a_gradient_that_misses_the_view_contract(Fn):
    """The upstream gradient of a concatenation on the last dim is a narrowed view one float past a 16-byte boundary."""
    Lq, Lk, B, heads, d = 8, 300, 2, 2, 32
    q, k, v, go, mask, allowed = cuda(*draw(Lq, Lk, B, heads, d, 161))
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    out = torch.cat([torch.zeros(Lq, B, 1, device="cuda"), Fn.masked_attention(*leaves, heads, mask, allowed)], dim=-1)
    wide = torch.cat([torch.zeros(Lq, B, 1, device="cuda"), go], dim=-1)
    grads = torch.autograd.grad(out, leaves, wide)
    want = Fn.masked_attention_backward(q, k, v, go, heads, mask, allowed)
    assert all(torch.equal(g, w) for g, w in zip(grads, want))


def test_bool_masks_are_read_as_uint8(Fn):
    q, k, v, go, mask, allowed = cuda(*draw(6, 35, 2, 2, 32, 171))
    want = Fn.masked_attention_backward(q, k, v, go, 2, mask, allowed)
    got = Fn.masked_attention_backward(q, k, v, go, 2, mask.bool(), allowed)
    assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_refusals_are_host_side(Fn):
    heads, d = 2, 32
    C = heads * d
    z = lambda L, c=C, **kw: torch.zeros(L, 2, c, device="cuda", **kw)
    m = lambda Lq, Lk, **kw: torch.zeros(2, Lq, Lk, dtype=torch.uint8, device="cuda", **kw)
    cnt = torch.full((2, 4), 8, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="allowed_count"):
        Fn.masked_attention_backward(z(4), z(8), z(8), z(4), heads, m(4, 8))
    with pytest.raises(RuntimeError, match="allowed_count"):
        Fn.masked_attention(z(4).requires_grad_(), z(8), z(8), heads, m(4, 8))
    with pytest.raises(RuntimeError, match="256"):
        Fn.masked_attention_backward(z(257), z(8), z(8), z(257), heads)
    with pytest.raises(RuntimeError, match="256"):
        Fn.masked_attention(z(257).requires_grad_(), z(8), z(8), heads)
    with pytest.raises(RuntimeError, match="32 or 64"):
        Fn.masked_attention_backward(z(4, 32), z(8, 32), z(8, 32), z(4, 32), 2)
    with pytest.raises(RuntimeError, match="float32"):
        Fn.masked_attention_backward(z(4), z(8), z(8, dtype=torch.float64), z(4), heads)
    with pytest.raises(RuntimeError, match="inner stride"):
        Fn.masked_attention_backward(z(4, 2 * C)[..., ::2], z(8), z(8), z(4), heads)
    with pytest.raises(RuntimeError, match=r"\(B, Lq, Lk\)"):
        Fn.masked_attention_backward(z(4), z(8), z(8), z(4), heads, m(4, 9), cnt)
    with pytest.raises(RuntimeError, match="mask must be"):
        Fn.masked_attention_backward(z(4), z(8), z(8), z(4), heads, m(4, 8).float(), cnt)
    with pytest.raises(RuntimeError, match="allowed_count must be"):
        Fn.masked_attention_backward(z(4), z(8), z(8), z(4), heads, m(4, 8), cnt.long())
    with pytest.raises(RuntimeError, match="mask"):                   # functions.attention keeps its refusal
        Fn.attention(z(4).requires_grad_(), z(8), z(8), heads, mask=m(4, 8), allowed_count=cnt)
    with pytest.raises(RuntimeError, match="256"):
        Fn.attention(z(4).requires_grad_(), z(257), z(257), heads)
