"""csrc/postprocess.hip at the places random logits of a handful of shapes do not reach: every instance and branch of the
semantic arg-max and the shared-memory gate of its MFMA form (a), exact ties in all three "first maximum wins" (b, c), the
sigmoid's saturated and denormal ranges (d), a second grid-stride sweep in isolation (e), the K = 256 areas table, the refusals and
the empty calls (f), and the three operand layouts of the "(K, T, h, w) view with contiguous maps" contract (g).

The reference is the torch CPU sequence interpolate -> crop -> sigmoid -> interpolate (postprocess_cases._cpu_sequence); decisions
on the same logits compare with intcmp.exact, semantic class sums with intcmp.near_boundary against the fp64 einsum at the
tolerance of test_postprocess_gpu.py.  Every case first asserts, from functions.postprocess_plan (the host function the launch
consults), that it runs the code it is here for.  All maps are a few thousand pixels except section e."""
import pytest
import torch

import intcmp
import postprocess_cases as PC
from postprocess_cases import S1, S2, GEN, _cpu_sequence, _logits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fn():
    from dvis_plus_amd import functions as Fn
    return Fn


def _vps_exact(logits, scores, geom, tag):
    hw, first, img, out = geom
    ids, conf, areas = _fn().vps_argmax(logits.to(DEV), scores.to(DEV), first, img, out)
    r_ids, r_conf, r_areas, m = PC.vps_reference(logits, scores, first, img, out)
    assert ids.dtype == torch.int32 and conf.dtype == torch.bool and areas.dtype == torch.int32
    intcmp.exact(ids.long(), r_ids, "vps_argmax ids " + tag)
    intcmp.exact(conf, r_conf, "vps_argmax conf " + tag)
    intcmp.exact(areas.long(), r_areas, "vps_argmax areas " + tag)
    return ids.cpu(), conf.cpu(), areas.cpu(), m


# ---- a. semantic dispatch ------------------------------------------------------------------------------------------------------
# Q, C, T, geometry, form, K4, second stage is the identity
VSS_DISPATCH = [
    (6, 70, 2, S1, "generic", 24, True),
    (10, 96, 1, S2, "generic", 24, False),
    (8, 65, 1, S1, "generic", 24, True),
    (12, 20, 2, S1, "generic", 8, True),            # Q % 4 == 0, but a row stride of 32
    (9, 40, 2, S2, "generic", 16, False),
    (7, 40, 1, S1, "generic", 16, True),            # K4 = 16 through the prefetching branch
    (124, 124, 1, S1, "mfma", 32, True),            # the last Q whose class matrix fits 64 KB of LDS
    (128, 124, 1, S1, "generic", 32, True),         # Q % 4 == 0, one step past the LDS gate
    (126, 124, 1, S1, "generic", 32, True),         # Q % 4 != 0
]


@pytest.mark.parametrize("Q,C,T,geom,form,K4,identity", VSS_DISPATCH)
def test_vss_argmax_every_instance_and_branch(Q, C, T, geom, form, K4, identity):
    Fn = _fn()
    hw, first, img, out = geom
    p = Fn.postprocess_plan("vss_argmax", Q, T, img, out, C)
    assert (p.form, p.K4, p.identity) == (form, K4, identity), p
    assert p.lds_bytes == (Q * 132 * 4 if form == "mfma" else 0) and p.sweeps == 1
    logits, cls = PC.vss_inputs(Q, C, T, hw)
    want, margin, tol, n_unsafe = PC.vss_reference(logits, cls, first, img, out)
    tag = f"vss_argmax {form} K4={K4} identity={identity} Q={Q} C={C} T={T} {hw}->{first}->{img}->{out}"
    intcmp._report(f"{tag}: the reference alone is undecided (fp32 CPU arg-max != fp64, or top-2 margin <= tol {tol:.2e}) at "
                   f"{n_unsafe} of {want.numel()} pixels")
    assert n_unsafe <= 4          # the allowance of 8 below must stay (nearly) unused by the reference: a flipped pixel fails on distance
    got = Fn.vss_argmax(logits.to(DEV), cls.to(DEV), first, img, out)
    assert got.dtype == torch.int64 and got.shape == want.shape
    intcmp.near_boundary(got, want, margin, tol, tag + " vs fp64 class sums", max_count=8)


# ---- b. exact ties in the semantic arg-max -------------------------------------------------------------------------------------
# In the MFMA form class c sits in accumulator tile c // 16, lane group (c % 16) // 4, register c % 4; a lane scans its own 32
# classes ascending, then the four lane groups merge over two shuffles (group 0 <-> 1 and 2 <-> 3, then 0 <-> 2).  The merge needs
# its index comparison exactly where the HIGHER class sits in a LOWER lane group than its twin.
TIE_PAIRS = [
    (5, 18),      # groups 1 and 0: the higher class in the lower group, met at the first shuffle
    (3, 64),      # one lane (group 0, tiles 0 and 4): decided inside the lane
    (17, 20),     # groups 0 and 1 of tile 1: the lower class in the lower group
    (0, 123),     # the two ends
    (9, 34),      # groups 2 and 0: the higher class in the lower group, met at the second shuffle
    (13, 22),     # groups 3 and 1: both arrive at the second shuffle as their neighbours' best
]
TIE_FORMS = [("mfma", 100), ("generic", 6)]


def _tie_run(Q, C, cls, form):
    Fn = _fn()
    hw, first, img, out = S1
    T = 2
    p = Fn.postprocess_plan("vss_argmax", Q, T, img, out, C)
    assert p.form == form and p.K4 == 32, p
    logits = _logits(Q, T, hw, 7 * Q + C)
    got = Fn.vss_argmax(logits.to(DEV), cls.to(DEV), first, img, out).cpu()
    return got, _cpu_sequence(logits, first, img, out, True)


@pytest.mark.parametrize("form,Q", TIE_FORMS)
@pytest.mark.parametrize("lo,hi", TIE_PAIRS)
def test_vss_argmax_tied_columns_first_wins(lo, hi, form, Q):
    C = 124
    cls = PC.tie_cls(Q, C, lo, hi, seed=1000 + 128 * lo + hi)
    assert torch.equal(cls[:, lo], cls[:, hi])
    got, m = _tie_run(Q, C, cls, form)
    # the pair is far above every other class at every pixel (fp64), so the answer is the pair's first column, no tolerance
    sem = PC.class_sums64(cls, m)
    others = torch.cat([sem[:lo], sem[lo + 1:hi], sem[hi + 1:]])
    pair_min, others_max = float(sem[lo].min()), float(others.max())
    intcmp._report(f"vss_argmax {form} Q={Q} tie ({lo}, {hi}): pair class sum >= {pair_min:.3g}, every other <= {others_max:.3g}; "
                   f"{int((got != lo).sum())} of {got.numel()} pixels are not {lo} ({int((got == hi).sum())} are {hi})")
    assert torch.equal(sem[lo], sem[hi]) and pair_min > 10 * others_max
    assert torch.equal(got, torch.full_like(got, lo))


@pytest.mark.parametrize("form,Q", TIE_FORMS)
def test_vss_argmax_all_columns_tied(form, Q):
    C = 124
    g = torch.Generator().manual_seed(Q)
    cls = (torch.rand(Q, generator=g) * 0.5 + 0.5).view(Q, 1).repeat(1, C)
    got, _ = _tie_run(Q, C, cls, form)
    assert torch.equal(got, torch.zeros_like(got)), f"{int((got != 0).sum())} pixels; values {got.unique().tolist()}"
    cls[:, 0] *= 0.5                              # now 1..C-1 tie above 0
    got, _ = _tie_run(Q, C, cls, form)
    assert torch.equal(got, torch.ones_like(got)), f"{int((got != 1).sum())} pixels; values {got.unique().tolist()}"


# ---- c. exact ties in the panoptic arg-max -------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 18])          # 18 frames: 16 planes in torch's vector-lane order + 2 in the scalar-tail order
def test_vps_argmax_copied_candidate_never_wins(T):
    K = 5
    hw = S2[0]
    base = _logits(K, T, hw, K * 10 + T).contiguous()
    base[4] = base[1]
    logits = PC.tk_view(base)
    scores = torch.rand(K, generator=torch.Generator().manual_seed(K)) * 0.5 + 0.5
    scores[4] = scores[1]
    ids, conf, areas, m = _vps_exact(logits, scores, S2, f"tie K={K} T={T} S2")
    assert torch.equal(m[4], m[1])
    assert int((ids == 1).sum()) > 0              # candidate 1 does win pixels: at each of them candidate 4 ties
    assert int((ids == 4).sum()) == 0 and int(areas[0, 4]) == 0 and int(areas[2, 4]) == 0
    assert int(areas[1, 4]) == int(areas[1, 1]) > 0


@pytest.mark.parametrize("T", [2, 18])
def test_vps_argmax_all_scores_zero(T):
    K = 5
    logits = _logits(K, T, S2[0], K * 10 + T + 1)
    ids, conf, areas, m = _vps_exact(logits, torch.zeros(K), S2, f"zero scores K={K} T={T} S2")
    assert int((ids != 0).sum()) == 0
    assert torch.equal(conf, m[0] >= 0.5)
    assert int(areas[0, 0]) == ids.numel() and int(areas[0, 1:].sum()) == 0


# ---- d. saturation -------------------------------------------------------------------------------------------------------------
SATURATION = [(6, 2, S2), (6, 18, S2), (6, 2, GEN)]


def _saturating(K, T, geom):
    hw, first, img, out = geom
    logits = PC.saturating_logits(K, T, hw, K * 100 + T)
    x = PC.stage_one(logits, first, img)
    # the sigmoid's arguments cover both cut-offs of the exp and the range between "denormal" and "zero"
    assert bool((x < -100).any()) and bool((x > 100).any()) and bool(((x > -104) & (x < -87)).any())
    return logits


@pytest.mark.parametrize("K,T,geom", SATURATION)
def test_resize2_floats_at_saturation(K, T, geom):
    Fn = _fn()
    hw, first, img, out = geom
    logits = _saturating(K, T, geom)
    tag = f"saturated K={K} T={T} {hw}->{first}->{img}->{out}"
    want = _cpu_sequence(logits, first, img, out, False)
    got = Fn.resize2(logits.to(DEV), first, img, out, sigmoid=False).cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "resize2 floats " + tag

    want = _cpu_sequence(logits, first, img, out, True)
    got = Fn.resize2(logits.to(DEV), first, img, out, sigmoid=True).cpu()
    diff = got.view(torch.int32) != want.view(torch.int32)
    n = int(diff.sum())
    tiny = torch.finfo(torch.float32).tiny
    denormal = (want != 0) & (want.abs() < tiny)
    n_den, n_den_diff = int(denormal.sum()), int((diff & denormal).sum())
    intcmp._report(f"resize2 sigmoid floats {tag}: {n} of {got.numel()} floats differ bitwise; max |d| "
                   f"{float((got - want).abs().max()):.2e}; torch has {int((want == 0).sum())} zeros, {int((want == 1).sum())} ones and "
                   f"{n_den} denormals, of which {n_den_diff} differ (the kernel returns {int(((got != 0) & (got.abs() < tiny)).sum())} "
                   f"denormals)")
    assert n_den > 0              # torch's CPU keeps denormals: 1 / (1 + e) must survive as it does there
    # the rule of test_resize2_floats_bitwise_vs_torch_cpu, unchanged (denormals included: none beyond it)
    assert n <= max(4, got.numel() // 10000) and float((got - want).abs().max()) <= 1.2e-7
    assert torch.equal(got == 0, want == 0), f"{int(((got == 0) != (want == 0)).sum())} elements are zero in one result only"
    assert torch.equal(got == 1, want == 1), f"{int(((got == 1) != (want == 1)).sum())} elements are one in one result only"


@pytest.mark.parametrize("K,T,geom", SATURATION)
def test_decisions_at_saturation(K, T, geom):
    Fn = _fn()
    hw, first, img, out = geom
    logits = _saturating(K, T, geom)
    tag = f"saturated K={K} T={T} {hw}->{first}->{img}->{out}"
    got = Fn.resize2_gt0(logits.to(DEV), first, img, out)
    intcmp.exact(got, _cpu_sequence(logits, first, img, out, False) > 0, "resize2_gt0 " + tag)
    scores = torch.rand(K, generator=torch.Generator().manual_seed(K)) * 0.5 + 0.5
    _vps_exact(logits, scores, geom, tag)


# ---- e. several sweeps ---------------------------------------------------------------------------------------------------------
def _sweep_case(name):
    op, K, T, geom, C = PC.SWEEP_CASES[name]
    p = _fn().postprocess_plan(op, K, T, geom[2], geom[3], C)
    assert p.sweeps >= 2, p
    return K, T, geom, C, p


def test_vps_argmax_second_sweep():
    K, T, geom, _, p = _sweep_case("vps_argmax")
    logits = _logits(K, T, geom[0], K * 10 + T)
    scores = torch.rand(K, generator=torch.Generator().manual_seed(K)) * 0.5 + 0.5
    _vps_exact(logits, scores, geom, f"{p.sweeps} sweeps K={K} T={T} {geom}")


@pytest.mark.parametrize("name,form", [("vss_argmax-generic", "generic"), ("vss_argmax-mfma", "mfma")])
def test_vss_argmax_second_sweep(name, form):
    Q, T, geom, C, p = _sweep_case(name)
    assert p.form == form, p
    hw, first, img, out = geom
    logits, cls = PC.vss_inputs(Q, C, T, hw)
    want, margin, tol, n_unsafe = PC.vss_reference(logits, cls, first, img, out, band=64)
    tag = f"vss_argmax {form} {p.sweeps} sweeps Q={Q} C={C} T={T} {hw}->{first}->{img}->{out}"
    intcmp._report(f"{tag}: the reference alone is undecided at {n_unsafe} of {want.numel()} pixels (tol {tol:.2e})")
    got = _fn().vss_argmax(logits.to(DEV), cls.to(DEV), first, img, out)
    assert got.shape == want.shape
    intcmp.near_boundary(got, want, margin, tol, tag + " vs fp64 class sums", max_count=8)


@pytest.mark.parametrize("sigmoid", [False, True])
def test_resize2_second_sweep(sigmoid):
    K, T, geom, _, p = _sweep_case("resize2")
    hw, first, img, out = geom
    logits = _logits(K, T, hw, K * 100 + T)
    want = _cpu_sequence(logits, first, img, out, sigmoid)
    got = _fn().resize2(logits.to(DEV), first, img, out, sigmoid=sigmoid).cpu()
    n = int((got.view(torch.int32) != want.view(torch.int32)).sum())
    intcmp._report(f"resize2 {p.sweeps} sweeps sigmoid={sigmoid} K={K} T={T} {geom}: {n} of {got.numel()} floats differ bitwise; "
                   f"max |d| {float((got - want).abs().max()):.2e}")
    if sigmoid:
        assert n <= max(4, got.numel() // 10000) and float((got - want).abs().max()) <= 1.2e-7
    else:
        assert n == 0


def test_resize2_gt0_second_sweep():
    K, T, geom, _, p = _sweep_case("resize2_gt0")
    hw, first, img, out = geom
    logits = _logits(K, T, hw, K * 100 + T + 1)
    got = _fn().resize2_gt0(logits.to(DEV), first, img, out)
    intcmp.exact(got, _cpu_sequence(logits, first, img, out, False) > 0, f"resize2_gt0 {p.sweeps} sweeps K={K} T={T} {geom}")


# ---- f. boundaries and refusals ------------------------------------------------------------------------------------------------
def test_vps_argmax_full_areas_table():
    K, T = 256, 1
    logits = _logits(K, T, S1[0], K * 10 + T)
    scores = torch.rand(K, generator=torch.Generator().manual_seed(K)) * 0.5 + 0.5
    ids, conf, areas, m = _vps_exact(logits, scores, S1, f"K={K} T={T} S1")
    assert areas.shape == (3, 256) and int(areas[0].sum()) == ids.numel() and int(areas[1, 255]) > 0


def test_sizes_past_the_tables_are_refused():
    Fn = _fn()
    hw, first, img, out = S1
    with pytest.raises(RuntimeError, match=r"K must be 1\.\.256"):
        Fn.vps_argmax(_logits(257, 1, hw, 0).to(DEV), torch.ones(257, device=DEV), first, img, out)
    with pytest.raises(RuntimeError, match=r"C must be 1\.\.128"):
        Fn.vss_argmax(_logits(4, 1, hw, 0).to(DEV), torch.ones(4, 129, device=DEV), first, img, out)
    torch.cuda.synchronize()


def _sentinel_empty(real):
    def filled(*a, **k):
        t = real(*a, **k)
        if t.is_floating_point():
            return t.fill_(float("nan"))
        return t.fill_(True) if t.dtype == torch.bool else t.fill_(0xAB if t.dtype == torch.uint8 else -7)
    return filled


def test_empty_calls(monkeypatch):
    """T = 0 (all four) and K = 0 (the resizes): correctly shaped empty outputs; the panoptic areas are zeroed although nothing else
    runs.  torch.empty hands out sentinel-filled memory for the calls."""
    Fn = _fn()
    hw, first, img, out = S2
    K = 5
    none = _logits(K, 0, hw, 0).to(DEV)
    assert none.shape == (K, 0, *hw)
    monkeypatch.setattr(torch, "empty", _sentinel_empty(torch.empty))
    ids, conf, areas = Fn.vps_argmax(none, torch.ones(K, device=DEV), first, img, out)
    sem = Fn.vss_argmax(none, torch.ones(K, 7, device=DEV), first, img, out)
    floats = [Fn.resize2(none, first, img, out, sigmoid=s) for s in (False, True)]
    masks = Fn.resize2_gt0(none, first, img, out)
    nocand = _logits(1, 2, hw, 0).to(DEV)[:0]
    assert nocand.shape == (0, 2, *hw)
    floats0 = Fn.resize2(nocand, first, img, out, sigmoid=True)
    masks0 = Fn.resize2_gt0(nocand, first, img, out)
    monkeypatch.undo()
    assert ids.shape == conf.shape == sem.shape == (0, *out)
    assert (ids.dtype, conf.dtype, sem.dtype) == (torch.int32, torch.bool, torch.int64)
    assert areas.shape == (3, K) and areas.dtype == torch.int32 and int((areas != 0).sum()) == 0, areas
    assert all(f.shape == (K, 0, *out) and f.dtype == torch.float32 for f in floats)
    assert masks.shape == (K, 0, *out) and masks.dtype == torch.bool
    assert floats0.shape == masks0.shape == (0, 2, *out) and masks0.dtype == torch.bool


# ---- g. operand layouts --------------------------------------------------------------------------------------------------------
def _in_layouts(values):
    tensors = [(name, make(DEV)) for name, make in PC.layouts(values)]
    (_, a), (_, b), (_, c) = tensors
    K, T, h, w = values.shape
    assert a.stride() == (h * w, K * h * w, w, 1) and b.stride() == (T * h * w, h * w, w, 1) and c.stride() == (2 * T * h * w, h * w, w, 1)
    assert c.storage_offset() == T * h * w
    assert all(torch.equal(t.cpu(), values) for _, t in tensors)
    return tensors


def test_three_layouts_same_bits():
    Fn = _fn()
    K, T = 5, 2
    hw, first, img, out = S2
    values = _logits(K, T, hw, 321).contiguous()
    scores = (torch.rand(K, generator=torch.Generator().manual_seed(K)) * 0.5 + 0.5).to(DEV)
    results = {}
    for name, t in _in_layouts(values):
        results[name] = [*Fn.vps_argmax(t, scores, first, img, out), Fn.resize2_gt0(t, first, img, out),
                         Fn.resize2(t, first, img, out, sigmoid=False), Fn.resize2(t, first, img, out, sigmoid=True)]
    ref = results.pop("tk-permuted")
    for name, res in results.items():
        for i, (x, y) in enumerate(zip(ref, res)):
            assert torch.equal(x.view(torch.int32) if x.is_floating_point() else x, y.view(torch.int32) if y.is_floating_point() else y), \
                (name, i)
    # and the values are the torch sequence's (one layout suffices: the others have its bits)
    intcmp.exact(ref[3], _cpu_sequence(values, first, img, out, False) > 0, "resize2_gt0, layouts case")
    r_ids, r_conf, r_areas, _ = PC.vps_reference(values, scores.cpu(), first, img, out)
    intcmp.exact(ref[0].long(), r_ids, "vps_argmax ids, layouts case")
    intcmp.exact(ref[2].long(), r_areas, "vps_argmax areas, layouts case")


@pytest.mark.parametrize("Q,C,geom,form", [(8, 100, S1, "mfma"), (5, 40, S2, "generic"), (6, 20, S1, "generic")])
def test_vss_argmax_three_layouts_same_bits(Q, C, geom, form):
    Fn = _fn()
    T = 2
    hw, first, img, out = geom
    assert Fn.postprocess_plan("vss_argmax", Q, T, img, out, C).form == form
    logits, cls = PC.vss_inputs(Q, C, T, hw)
    values = logits.contiguous()
    got = {name: Fn.vss_argmax(t, cls.to(DEV), first, img, out) for name, t in _in_layouts(values)}
    assert torch.equal(got["tk-permuted"], got["contiguous"]) and torch.equal(got["tk-permuted"], got["every-second"])
    want, margin, tol, _ = PC.vss_reference(values, cls, first, img, out)
    intcmp.near_boundary(got["tk-permuted"], want, margin, tol, f"vss_argmax {form}, layouts case Q={Q} C={C}", max_count=8)
