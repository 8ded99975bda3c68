"""csrc/attention.hip at its dispatch, tile, mask and range edges.

Every case first asserts ``functions.attention_plan`` — the kernel that serves it and, where the case was chosen for it, the number of
key splits, of query chunks and the key count of the last split — and then compares with the fp64 ``ref_attention`` of
tests/test_attention_gpu.py at that file's tolerance (2e-5 abs on O(1) outputs).  The plan comes from the function the launch
itself consults, so a moved threshold fails the plan assertion instead of silently moving the case to another kernel.

Outputs are written into NaN-filled buffers: a row the kernel never stores fails the comparison whatever the allocator left there.

One-hot cases: each query i has a target key pi(i) whose score exceeds every other score of its row by >= 200 log2 units, so every
other probability underflows to exactly 0 in fp32 and out[i] must equal v[pi(i)] bit for bit, on every kernel and through both
merges.  Score-range cases: rows whose maxima run from about -900 to +900 log2 units with an ordinary N(0, 1) spread inside each
row; close competitors at |s| ~ 900 make the rounding of an fp32 score visible in the probabilities, so the bound is measured:
max(2e-5, 4 x e32), e32 = the error of fp32 ``cpu_ops.attention`` against fp64 on the same inputs (4 = the project's factor for a
different summation order, tests/test_attention_backward_gpu.py).  It is never derived from the kernel's own output.  Both kinds
assert their precondition on the CPU reference before the GPU is touched."""
import math

import pytest
import torch

from test_attention_gpu import ref_attention

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5
B, H = 2, 2

FWD, SHORT, KEYSPLIT = "attn_fwd_kernel", "attn_short_kernel", "attn_keysplit_kernel"


@pytest.fixture(scope="module")
def Fn():
    from dvis_plus_amd import functions
    return functions


def last_split_keys(plan, Lk):
    return Lk - (plan.nsplit - 1) * plan.keys_per_split


def check_plan(Fn, q, k, mask, kernel, short=False):
    """The plan of the call, after the assertions every case shares: the kernel, the query chunks for its chunk size, and splits that
    tile the keys (every split but the last full, the last one non-empty)."""
    Lq, Lk = q.shape[0], k.shape[0]
    plan = Fn.attention_plan(q, k, H, mask, short)
    assert plan.kernel == kernel, (Lq, Lk, plan)
    per_chunk = {FWD: 128, SHORT: 16, KEYSPLIT: 112}[kernel]
    assert plan.qchunks == -(-Lq // per_chunk), plan
    assert 0 < last_split_keys(plan, Lk) <= plan.keys_per_split, plan
    if kernel == SHORT:
        assert plan.nsplit == 1
    return plan


def run(Fn, q, k, v, mask=None, allowed=None, short=False):
    out = torch.full(q.shape, float("nan"), device=DEV)
    dev = lambda t: None if t is None else t.to(DEV)
    got = Fn.attention(q.to(DEV), k.to(DEV), v.to(DEV), H, dev(mask), dev(allowed), out=out, short=short)
    assert got is out
    return out.cpu()


def draw(Lq, Lk, d, masked, seed, nb=B):
    """Operands as tests/test_attention_gpu.py draws them; the mask keeps key 0 of every row and leaves one row a single live key."""
    g = torch.Generator().manual_seed(seed)
    C = H * d
    q, k, v = (torch.randn(L, nb, C, generator=g) for L in (Lq, Lk, Lk))
    q = q * 2.0
    mask = None
    if masked:
        mask = torch.rand(nb, Lq, Lk, generator=g) < 0.7
        mask[:, :, 0] = False
        mask[0, 0, 1:] = True
    return q, k, v, mask


def compare(Fn, Lq, Lk, d, masked, kernel, seed=0):
    q, k, v, mask = draw(Lq, Lk, d, masked, seed + 7 * Lq + Lk)
    plan = check_plan(Fn, q, k, mask, kernel)
    ref = ref_attention(q, k, v, H, mask)
    out = run(Fn, q, k, v, mask)
    err = (out.double() - ref).abs().max().item()
    assert err <= TOL, f"Lq {Lq} Lk {Lk} d {d} masked {masked}: err {err:.3e} ({plan})"      # (NaN fails: a row never stored)
    return plan


# ------------------------------------------------------------------------------------------------------------------------------
# Query-partitioned kernel (attn_fwd_kernel): 128 queries per workgroup (8 waves of 16), keys in LDS stages of 64 (d = 32) / 32
# (d = 64), tiles of 16 keys, optional split over keys.  Lk: tails of 1 (129, 257) and 3 (131, 255, 511) keys, a 4-aligned mask
# row with a partial last tile (132), ragged last LDS stages; Lq: waves switched off (1, 16, 17), a second query chunk with one
# live row (129), full and almost full chunks.
FWD_LK = [129, 131, 132, 255, 256, 257, 511]
FWD_LQ = [1, 16, 17, 112, 113, 128, 129]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("Lk", FWD_LK)
def test_query_partitioned_lattice(Fn, Lk, d, masked):
    for Lq in FWD_LQ:
        plan = compare(Fn, Lq, Lk, d, masked, FWD)
        assert plan.nsplit * plan.keys_per_split >= Lk
        if Lk in (129, 257):
            assert last_split_keys(plan, Lk) % 16 == 1           # the last tile of the last split holds one key
        if Lq == 129:
            assert plan.qchunks == 2


@pytest.mark.parametrize("Lq,Lk,masked", [(64, 513, False), (64, 513, True), (33, 1024, False), (33, 1024, True),
                                          (100, 627, True), (200, 1035, True)])
def test_query_partitioned_long_keys_at_head_dim_32(Fn, Lq, Lk, masked):
    """d = 32 with >= 512 keys stays on the query-partitioned kernel at <= 64 queries, and under a mask whose rows are not 4-byte
    aligned (Lk % 4 != 0: the decoder's stride-32 level after test-time resizing, 19 x 33 = 627, 23 x 45 = 1035)."""
    plan = compare(Fn, Lq, Lk, 32, masked, FWD)
    assert plan.nsplit > 1
    if (Lq, Lk) == (200, 1035):
        assert plan.qchunks == 2 and last_split_keys(plan, Lk) == 11       # a last split that is one partial tile


# ------------------------------------------------------------------------------------------------------------------------------
# Key-partitioned kernel (attn_keysplit_kernel): d = 32, > 64 queries, >= 512 keys, a mask only with Lk % 4 == 0.  A wave owns a
# key range and 7 query tiles (112 queries): Lq 65 (one live row in the fifth tile), 112 / 113 and 224 / 225 (a further query chunk
# with one live row).
KS_LQ = [65, 112, 113, 224, 225]


@pytest.mark.parametrize("Lk,masked", [(512, True), (516, True), (532, True), (1000, True), (513, False), (1025, False)])
def test_key_partitioned_lattice(Fn, Lk, masked):
    for Lq in KS_LQ:
        plan = compare(Fn, Lq, Lk, 32, masked, KEYSPLIT)
        assert plan.nsplit > 1 and plan.keys_per_split % 16 == 0
        if Lk == 1025:
            assert last_split_keys(plan, Lk) == 17     # one full tile + one key: the odd-tile exit of the ping-pong loop
        if Lq in (113, 225):
            assert plan.qchunks == Lq // 112 + 1


# ------------------------------------------------------------------------------------------------------------------------------
# Short kernel (attn_short_kernel): Lk <= 128, a workgroup per 16 queries, key tile kt on wave kt % 4: at Lk <= 48 some waves own
# no key tile; 49 / 64 / 65 / 112 / 113 walk the second tile of each wave in.
SHORT_LK = [1, 2, 15, 16, 17, 48, 49, 64, 65, 112, 113, 127, 128]
SHORT_LQ = [1, 16, 17, 100]


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("Lk", SHORT_LK)
def test_short_lattice(Fn, Lk, d):
    for Lq in SHORT_LQ:
        for masked in (False, True):
            compare(Fn, Lq, Lk, d, masked, SHORT)


def test_pinned_short_kernel_is_the_default_kernel_below_129_keys(Fn):
    q, k, v, mask = draw(17, 113, 32, True, 5)
    assert check_plan(Fn, q, k, mask, SHORT, short=True) == check_plan(Fn, q, k, mask, SHORT)
    assert torch.equal(run(Fn, q, k, v, mask, short=True), run(Fn, q, k, v, mask))
    with pytest.raises(RuntimeError, match="128"):
        Fn.attention_plan(q, torch.zeros(129, B, 64), H, short=True)


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq,Lk,d,kernel", [(100, 405, 32, FWD), (100, 627, 32, FWD), (130, 257, 64, FWD), (113, 532, 32, KEYSPLIT),
                                            (17, 113, 32, SHORT)])
def test_rows_blocked_everywhere_ignore_their_mask_on_every_kernel(Fn, Lq, Lk, d, kernel):
    """dvis_Plus/video_mask2former_transformer_decoder.py:297 with allowed_count from the mask: the first and the last query blocked
    everywhere (they attend to every key), next to rows whose only live key is the last key of the last split, or key 0."""
    q, k, v, _ = draw(Lq, Lk, d, False, 11)
    mask = torch.rand(B, Lq, Lk, generator=torch.Generator().manual_seed(Lq + Lk)) < 0.5
    mask[0, 0] = True
    mask[B - 1, Lq - 1] = True
    mask[0, 1] = True
    mask[0, 1, Lk - 1] = False
    mask[B - 1, Lq - 2] = True
    mask[B - 1, Lq - 2, 0] = False
    mask[B - 1, 2] = True
    mask[B - 1, 2, Lk - 1] = False
    allowed = (~mask).sum(-1).int()
    assert (allowed == 0).sum().item() == 2 and (allowed == 1).sum().item() == 3
    check_plan(Fn, q, k, mask, kernel)
    fixed = mask.clone()
    fixed[torch.where(fixed.sum(-1) == fixed.shape[-1])] = False
    ref = ref_attention(q, k, v, H, fixed)
    out = run(Fn, q, k, v, mask, allowed)
    err = (out.double() - ref).abs().max().item()
    assert err <= TOL, f"err {err:.3e}"
    assert torch.equal(out[1, 0], v[Lk - 1, 0]) and torch.equal(out[Lq - 2, B - 1], v[0, B - 1])      # one live key: exact


# ------------------------------------------------------------------------------------------------------------------------------
def scores_log2(q, k, d):
    """fp64 scores in the kernels' log2 units, (B, H, Lq, Lk)."""
    Lq, nb, _ = q.shape
    qh = q.double().view(Lq, nb, H, d).permute(1, 2, 0, 3)
    kh = k.double().view(k.shape[0], nb, H, d).permute(1, 2, 0, 3)
    return (qh @ kh.transpose(-1, -2)) * (math.log2(math.e) / d ** 0.5)


def one_hot_inputs(Lq, Lk, d, seed, integer_v=False, nb=B):
    """q, k, v, pi (nb, Lq): keys are random directions of one length, q_i lies along k[pi(i)]; the length comes from the largest
    cosine between two keys of a (batch entry, head), so that the target's score leads its row by 256 log2 units (asserted >= 200 by
    the caller on the fp64 scores).  pi is random with repeats — not monotone — and reaches the first and the last key."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(Lk, nb, H, d, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    uh = u.permute(1, 2, 0, 3)
    cos = uh @ uh.transpose(-1, -2)
    cos.diagonal(dim1=-2, dim2=-1).fill_(-1.0)
    cmax = cos.max().item() if Lk > 1 else 0.0
    a = math.sqrt(256.0 * d ** 0.5 / (math.log2(math.e) * (1.0 - cmax)))
    pi = torch.randint(0, Lk, (nb, Lq), generator=g)
    pi[:, 0] = Lk - 1
    pi[:, Lq - 1] = 0
    pi[0, Lq // 2] = Lk - 1
    k = (a * u).float().reshape(Lk, nb, H * d)
    q = torch.stack([k[pi[b], b] for b in range(nb)], 1)                     # (Lq, nb, C)
    if integer_v:
        v = torch.randint(-3, 4, (Lk, nb, H * d), generator=g).float()
    else:
        v = torch.randn(Lk, nb, H * d, generator=g)
    return q, k, v, pi


def one_hot_margin(q, k, d, pi):
    s = scores_log2(q, k, d)
    idx = pi[:, None, :, None].expand(-1, H, -1, 1)
    top = s.gather(-1, idx)
    rest = s.scatter(-1, idx, float("-inf")).amax(-1, keepdim=True)
    return (top - rest).min().item()


@pytest.mark.parametrize("Lq,Lk,d,kernel,variants", [
    (113, 1025, 32, KEYSPLIT, ("plain",)),                    # (a mask with Lk % 4 != 0 would leave this kernel)
    (113, 532, 32, KEYSPLIT, ("plain", "masked", "reset")),
    (129, 257, 64, FWD, ("plain", "masked", "reset")),
    (100, 627, 32, FWD, ("masked", "reset")),                 # (without a mask this shape is the key-partitioned kernel's)
    (17, 113, 32, SHORT, ("plain", "masked", "reset")),
    (17, 113, 64, SHORT, ("plain", "masked", "reset")),
])
def test_one_hot_attention_returns_the_chosen_value_rows_exactly(Fn, Lq, Lk, d, kernel, variants):
    from dvis_plus_amd import cpu_ops
    q, k, v, pi = one_hot_inputs(Lq, Lk, d, 31 + Lq + Lk + d)
    want = torch.stack([v[pi[b], b] for b in range(B)], 1)
    margin = one_hot_margin(q, k, d, pi)
    assert margin >= 200.0, margin
    g = torch.Generator().manual_seed(Lq * Lk)
    for variant in variants:
        mask = allowed = None
        if variant != "plain":
            mask = torch.rand(B, Lq, Lk, generator=g) < 0.7
            mask.scatter_(-1, pi[..., None], False)                # pi(i) stays live
            if variant == "reset":                                  # rows blocked everywhere, count 0: they still pick pi(i)
                mask[0, 0] = mask[B - 1, Lq - 1] = mask[0, Lq // 2] = True
                allowed = (~mask).sum(-1).int()
                assert (allowed == 0).sum().item() == 3
        # the reference alone must meet the claim: otherwise the inputs are wrong, not the kernel
        assert torch.equal(cpu_ops.attention(q, k, v, H, mask, allowed), want), variant
        check_plan(Fn, q, k, mask, kernel)
        out = run(Fn, q, k, v, mask, allowed)
        assert torch.equal(out, want), f"{variant}: {(out != want).any(-1).nonzero()[:8].tolist()} (query, batch) rows differ"


# ------------------------------------------------------------------------------------------------------------------------------
def score_range_inputs(Lq, Lk, d, seed, nb=B, span=900.0):
    """q_i = g_i + alpha_i u, k_j = h_j + beta u with h_j orthogonal to the unit vector u (one per batch entry and head): the score
    of (i, j) is g_i . h_j / sqrt(d) — an ordinary N(0, 1) spread within the row — plus a row constant that runs, over the queries in
    a shuffled order, from -span to +span log2 units."""
    g = torch.Generator().manual_seed(seed)
    f64 = dict(generator=g, dtype=torch.float64)
    u = torch.randn(1, nb, H, d, **f64)
    u = u / u.norm(dim=-1, keepdim=True)
    gq, hk = torch.randn(Lq, nb, H, d, **f64), torch.randn(Lk, nb, H, d, **f64)
    hk = hk - (hk * u).sum(-1, keepdim=True) * u
    gq = gq - (gq * u).sum(-1, keepdim=True) * u
    beta = 30.0
    t = torch.linspace(-span, span, Lq, dtype=torch.float64)[torch.randperm(Lq, generator=g)] if Lq > 1 else torch.tensor([span])
    alpha = (t * d ** 0.5 / (beta * math.log2(math.e))).view(Lq, 1, 1, 1)
    q = (gq + alpha * u).float().reshape(Lq, nb, H * d)
    k = (hk + beta * u).float().reshape(Lk, nb, H * d)
    v = torch.randn(Lk, nb, H * d, generator=g)
    return q, k, v


def assert_score_range(q, k, d, mask=None, span=900.0):
    s = scores_log2(q, k, d)
    if mask is not None:
        s = s.masked_fill(mask[:, None], float("-inf"))
    rowmax = s.amax(-1)
    assert rowmax.min().item() < -0.9 * span and rowmax.max().item() > 0.9 * span, (rowmax.min().item(), rowmax.max().item())
    spread = (s - s.mean(-1, keepdim=True)).std(-1) if mask is None else None
    if spread is not None:                                  # natural units: g_i . h_j / sqrt(d) is N(0, ~1)
        nat = spread / math.log2(math.e)
        assert 0.5 < nat.min().item() and nat.max().item() < 2.0, (nat.min().item(), nat.max().item())


@pytest.mark.parametrize("Lq,Lk,d,masked,kernel", [
    (113, 1025, 32, False, KEYSPLIT), (113, 532, 32, True, KEYSPLIT), (129, 257, 64, False, FWD), (100, 627, 32, True, FWD),
    (130, 257, 32, True, FWD), (17, 113, 32, False, SHORT), (33, 100, 64, True, SHORT),
])
def test_row_maxima_from_minus_900_to_plus_900_log2_units(Fn, Lq, Lk, d, masked, kernel):
    from dvis_plus_amd import cpu_ops
    q, k, v = score_range_inputs(Lq, Lk, d, 57 + Lq + Lk)
    mask = None
    assert_score_range(q, k, d)
    if masked:
        mask = torch.rand(B, Lq, Lk, generator=torch.Generator().manual_seed(Lk)) < 0.5
        mask[:, :, 0] = False
        assert_score_range(q, k, d, mask)
    ref = ref_attention(q, k, v, H, mask)
    e32 = (cpu_ops.attention(q, k, v, H, mask).double() - ref).abs().max().item()
    check_plan(Fn, q, k, mask, kernel)
    out = run(Fn, q, k, v, mask)
    err = (out.double() - ref).abs().max().item()
    print(f"score range {(Lq, Lk, d, masked)} {kernel}: e32 {e32:.3e} kernel err {err:.3e} ratio {err / max(e32, 1e-30):.2f}")
    assert err <= max(TOL, 4 * e32), (err, e32)
