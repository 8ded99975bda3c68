"""functions.mask_gemm_plan / dvis_mask_gemm_plan: how csrc/mask_gemm.hip cuts a call into passes, steps and workgroups and which
instantiation serves a pass, asked of the host function the launch itself consults (no GPU: only shapes are read).  The GPU file
(test_mask_gemm_edges_gpu.py) asserts its cases' plans; this one pins where the boundaries are, and checks the exact-integer cases
of mask_gemm_cases.py on the CPU: their exactness bound and that the planted rows and pixels do what they are planted for."""
import pytest
import torch

import mask_gemm_cases as MC


def plan(mode, B, Q, C, H, W, h=0, w=0, **kw):
    from dvis_plus_amd import functions as Fn
    return Fn.mask_gemm_plan(mode, B, Q, C, H, W, h, w, **kw)


@pytest.mark.parametrize("Q,qts,qbegs", [
    (1, (2,), (0,)), (32, (2,), (0,)), (33, (4,), (0,)), (64, (4,), (0,)), (65, (7,), (0,)), (100, (7,), (0,)), (112, (7,), (0,)),
    (113, (4, 4), (0, 64)), (129, (7, 4), (0, 80)), (200, (7, 7), (0, 112)), (224, (7, 7), (0, 112)),
    (225, (7, 7, 7), (0, 80, 160)), (256, (7, 7, 4), (0, 96, 192)), (300, (7, 7, 7), (0, 112, 224)),
])
def test_passes_by_queries(Q, qts, qbegs):
    for mode, size in ((0, (0, 0)), (1, (4, 6)), (2, (0, 0))):
        p = plan(mode, 2, Q, 32, 8, 12, *size)
        assert tuple(x.QT for x in p) == qts and tuple(x.qbeg for x in p) == qbegs, (mode, p)
    assert MC.passes_of(Q) == list(qbegs)           # the helper plants its rows at these edges
    # the tiles of the passes cover the queries: 200 -> 7 + 6, 225 -> 5 + 5 + 5, 300 -> 7 + 7 + 5
    tiles = [((qbegs[i + 1] if i + 1 < len(qbegs) else -(-Q // 16) * 16) - qbegs[i]) // 16 for i in range(len(qbegs))]
    assert all(t <= qt for t, qt in zip(tiles, qts)) and sum(tiles) == -(-Q // 16)
    assert {200: [7, 6], 225: [5, 5, 5], 300: [7, 7, 5], 113: [4, 4], 256: [6, 6, 4]}.get(Q, tiles) == tiles


@pytest.mark.parametrize("C", [1, 3, 4, 5, 16, 31, 32, 33, 40, 64, 100, 255, 256])
def test_fullc_and_vec(C):
    for mode in (0, 1, 2):
        for h, w in ((4, 8), (5, 13), (1, 6)):          # pixels % 4 == 0, odd, even but not % 4
            shape = (2 * h, 2 * w, h, w) if mode == 1 else (h, w)
            for aligned in (True, False):
                for embed_aligned in (True, False):
                    for p in plan(mode, 2, 33, C, *shape, aligned=aligned, embed_aligned=embed_aligned):
                        assert p.fullc == (C % 32 == 0 and embed_aligned)
                        assert p.vec == (mode != 1 and (h * w) % 4 == 0 and aligned and p.fullc)


@pytest.mark.parametrize("HW,gpf,spf,gpf1,spf1", [(1, 1, 1, 1, 1), (63, 1, 1, 4, 1), (64, 1, 1, 4, 1), (65, 2, 1, 5, 1),
                                                   (512, 8, 1, 32, 4), (513, 9, 2, 33, 5)])
def test_groups_and_steps_per_frame(HW, gpf, spf, gpf1, spf1):
    """A wave group is 64 map pixels (mode 1: 16 outputs), a step 8 groups of one frame."""
    for mode in (0, 2):
        (p,) = plan(mode, 3, 100, 32, 1, HW)
        assert (p.gpf, p.spf, p.total_steps) == (gpf, spf, 3 * spf)
    (p,) = plan(1, 3, 100, 32, 2, 2 * HW, 1, HW)
    assert (p.gpf, p.spf, p.total_steps) == (gpf1, spf1, 3 * spf1)


def test_workgroups_and_the_batch():
    """nwg = min(total_steps, 256 at seven query tiles, else 512); nothing but total_steps = B * spf (and with it nwg) reads B."""
    for mode, Q, H, W, size in [(0, 100, 80, 80, (0, 0)), (0, 20, 8, 8, (0, 0)), (0, 129, 48, 48, (0, 0)), (1, 100, 32, 64, (16, 32)),
                                (1, 20, 32, 64, (16, 32)), (2, 100, 16, 36, (0, 0)), (2, 50, 15, 7, (0, 0))]:
        one = plan(mode, 1, Q, 32, H, W, *size)
        for B in (1, 2, 40, 130, 255, 256, 257, 511, 512, 513, 520):
            many = plan(mode, B, Q, 32, H, W, *size)
            assert len(many) == len(one)
            for a, b in zip(one, many):
                assert b.total_steps == B * a.spf and b.nwg == min(b.total_steps, 256 if b.QT == 7 else 512)
                assert b._replace(total_steps=0, nwg=0) == a._replace(total_steps=0, nwg=0)


def test_plan_refuses_what_the_launch_refuses():
    with pytest.raises(RuntimeError, match="C <= 256"):
        plan(0, 1, 4, 257, 8, 8)
    with pytest.raises(RuntimeError, match="even integer"):
        plan(1, 1, 4, 32, 8, 16, 4, 4)              # H / h = 2, W / w = 4
    with pytest.raises(RuntimeError, match="even integer"):
        plan(1, 1, 4, 32, 9, 9, 3, 3)               # factor 3
    with pytest.raises(RuntimeError, match="mode"):
        plan(3, 1, 4, 32, 8, 8)


@pytest.mark.parametrize("name", sorted(MC.MULTI_STEP))
def test_multi_step_cases_are_multi_step_exact_and_planted(name):
    mode, B, Q, C, H, W, size, want = MC.MULTI_STEP[name]
    p = plan(mode, B, Q, C, H, W, *(size or (0, 0)))
    assert [(x.QT, x.spf, x.total_steps, x.nwg) for x in p] == want
    assert any(x.total_steps > x.nwg for x in p)
    case = MC.multi_step_case(name)
    values, zero_outputs = MC.multi_step_values(name, case)
    MC.assert_exact_outputs(values)
    kinds = MC.assert_planted(case, values)
    assert kinds == {MC.ZERO, MC.NEG, MC.BLOCKED}
    assert {q for _, q in case.planted} == set(MC.planted_positions(Q))
    MC.assert_multi_frame(case, values, zero_outputs)


def test_pooled_cases_on_the_cpu():
    """The two attn_mask_pooled cases that are no entry of MULTI_STEP: the single-step B = 130 form of the byte-store case, and (a
    few frames of) the case that goes through center_pool3 — its plan for all 130."""
    mode, B, Q, C, h, w, _, want = MC.POOLED_BYTE_STORES_130
    assert [(x.QT, x.spf, x.total_steps, x.nwg) for x in plan(mode, B, Q, C, h, w)] == want
    mode, B, Q, C, h, w, _, want = MC.POOLED_VEC
    (p,) = plan(mode, B, Q, C, h, w)
    assert [(p.QT, p.spf, p.total_steps, p.nwg)] == want and p.total_steps > p.nwg and p.vec and p.gpf == 9
    case = MC.pooled_vec_case(B=4)
    values = MC.reference_small(case.embed, case.feat, (h, w), chunk=2)
    MC.assert_exact_outputs(values)
    assert MC.assert_planted(case, values) == {MC.ZERO, MC.NEG, MC.BLOCKED}
    MC.assert_multi_frame(case, values, [h * w - 1])


@pytest.mark.parametrize("Q,positions", [(1, [0]), (16, [0, 15]), (17, [0, 15, 16]), (113, [0, 15, 16, 63, 64, 112]),
                                         (256, [0, 15, 16, 95, 96, 191, 192, 255])])
def test_planted_rows_at_small_and_multi_pass_queries(Q, positions):
    assert MC.planted_positions(Q) == positions
    case = MC.make_case(2, Q, 32, 8, 12, seed=Q)
    assert {q for _, q in case.planted} == set(positions)
    values = MC.reference_logits(case.embed, case.feat).flatten(2)
    MC.assert_exact_outputs(values)
    MC.assert_planted(case, values)
    MC.assert_multi_frame(case, values, case.zero_pixels)
    small = MC.reference_small(case.embed, case.feat, (4, 6))
    MC.assert_exact_outputs(small)
    MC.assert_planted(case, small)


def test_exactness_bound_is_checked():
    case = MC.make_case(1, 4, 8, 2, 2, seed=0)
    with pytest.raises(AssertionError):
        MC.assert_exact_inputs(case._replace(embed=case.embed + 0.5))
    with pytest.raises(AssertionError):
        MC.assert_exact_inputs(case._replace(feat=case.feat * 2 + 1))
    with pytest.raises(AssertionError):
        MC.assert_exact_outputs(torch.tensor([0.1], dtype=torch.float64))
