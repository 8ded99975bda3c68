"""Set criterion on CPU tensors: the cpu_ops formulations, the matchers and the criterion classes against the reference's
recorded results (tests/golden/g14_criterion.npz, written by gen_criterion_golden.py), border coordinates, target dtypes,
Q > G / Q = G / G = 0, and build_criterion against the reference's from_config (criterion_weight_dicts.json)."""
import json
import os

import numpy as np
import pytest
import torch

from criterion_cases import G14, GOLDEN, Replay, cost_terms_torch, point_losses_torch

from dvis_plus_amd import cpu_ops
from dvis_plus_amd import functions as Fn
from dvis_plus_amd.criterion import SetCriterion, VideoSetCriterion, build_criterion
from dvis_plus_amd.matcher import (HungarianMatcher, VideoHungarianMatcher, VideoHungarianMatcher_Consistent,
                                   linear_sum_assignment)

DEV = "cpu"
TOL = 1e-5      # fp32 formulations against the reference's fp32 results at these small shapes (terms of magnitude ~ 1)


@pytest.fixture(scope="module")
def g14():
    return G14()


def _matcher(g14, cls, **kw):
    return cls(num_points=g14.meta["K"], **g14.meta["weights"], **kw)


@pytest.mark.parametrize("case", ["video", "image"])
def test_cost_terms_and_indices_match_the_reference(g14, case):
    image = g14.meta["cases"][case]["image"]
    out, tg = g14.outputs(case, DEV, layers=1), g14.targets(case, DEV)
    w = g14.meta["weights"]
    for b, t in enumerate(tg):
        C, terms = Fn.match_cost(out["pred_masks"][b], t["masks"], g14.t(case, f"match_draw_{b}"), out["pred_logits"][b],
                                 t["labels"], w["cost_class"], w["cost_mask"], w["cost_dice"], return_terms=True)
        ref_terms, ref_C = g14.t(case, f"match_terms_{b}"), g14.t(case, f"match_C_{b}")
        assert terms.shape == ref_terms.shape and C.shape == ref_C.shape
        if C.numel():
            assert (terms - ref_terms).abs().max() <= TOL
            assert (C - ref_C).abs().max() <= 12 * TOL      # 5 + 5 + 2 times the terms' bound
    m = _matcher(g14, HungarianMatcher if image else VideoHungarianMatcher)
    m._rand = Replay([g14.t(case, f"match_draw_{b}") for b in range(len(tg))])
    idx = m(out, tg)
    assert len(idx) == len(tg)
    for b, (i, j) in enumerate(idx):
        assert i.dtype == j.dtype == torch.int64 and i.device.type == "cpu"
        assert np.array_equal(torch.stack((i, j)).numpy(), g14.t(case, f"match_idx_{b}").numpy()), (case, b)


def test_consistent_matcher_indices(g14):
    c = g14.meta["cases"]["consistent"]
    m = _matcher(g14, VideoHungarianMatcher_Consistent, frames=c["frames"])
    m._rand = Replay([g14.t("consistent", f"match_draw_{i}") for i in range(c["n_draws"])])
    idx = m(g14.outputs("consistent", DEV), g14.targets("consistent", DEV))
    assert len(idx) == 2
    for b, (i, j) in enumerate(idx):
        assert np.array_equal(torch.stack((i, j)).numpy(), g14.t("consistent", f"match_idx_{b}").numpy())


@pytest.mark.parametrize("case", ["video", "image"])
def test_criterion_losses_and_gradient(g14, case):
    c = g14.meta["cases"][case]
    n_aux = c["n_aux"]
    wd = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    wd.update({f"{k}_{i}": v for i in range(n_aux) for k, v in list(wd.items())[:3]})
    args = (g14.meta["NCLS"],)
    kw = dict(weight_dict=wd, eos_coef=0.1, losses=["labels", "masks"], num_points=g14.meta["K"], oversample_ratio=3.0,
              importance_sample_ratio=0.75)
    crit = SetCriterion(*args, matcher=_matcher(g14, HungarianMatcher), **kw) if c["image"] else \
        VideoSetCriterion(*args, matcher=_matcher(g14, VideoHungarianMatcher), **kw)
    assert tuple(crit.empty_weight.shape) == (g14.meta["NCLS"] + 1,) and float(crit.empty_weight[-1]) == pytest.approx(0.1)
    replay = Replay([g14.t(case, f"crit_draw_{i:02d}") for i in range(c["n_crit_draws"])])
    crit._rand = crit.matcher._rand = replay
    out = g14.outputs(case, DEV, requires_grad=True)
    losses = crit(out, g14.targets(case, DEV))
    assert replay.i == c["n_crit_draws"]
    assert sorted(losses) == c["loss_keys"]
    for k, v in losses.items():
        ref = float(g14.t(case, f"loss/{k}"))
        assert abs(float(v.detach()) - ref) <= TOL * max(1.0, abs(ref)), (k, float(v.detach()), ref)
    sum(losses[k] * wd[k] for k in losses).backward()
    g, ref = out["pred_masks"].grad, g14.t(case, "grad_pred_masks")
    if c["image"]:
        ref = ref[:, :, 0]
    assert (g - ref).abs().max() <= 1e-6 * max(1.0, float(ref.abs().max())) + 1e-8, float((g - ref).abs().max())


def test_ret_match_result_and_matcher_outputs(g14):
    crit = VideoSetCriterion(g14.meta["NCLS"], matcher=_matcher(g14, VideoHungarianMatcher),
                             weight_dict={"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}, eos_coef=0.1,
                             losses=["labels", "masks"], num_points=64, oversample_ratio=3.0, importance_sample_ratio=0.75)
    out, tg = g14.outputs("video", DEV), g14.targets("video", DEV)
    torch.manual_seed(0)
    losses, idx = crit(out, tg, matcher_outputs=g14.outputs("video", DEV, layers=1), ret_match_result=True)
    assert len(idx) == len(tg) and {"loss_ce", "loss_mask_1", "loss_dice_0"} <= set(losses)


def test_border_coordinates():
    g = torch.Generator().manual_seed(3)
    rows = torch.randn(2, 5, 7, generator=g)
    one = float(np.nextafter(np.float32(1), np.float32(0)))
    coords = torch.tensor([[0.0, 0.0], [one, one], [1.0, 1.0], [0.0, one], [-0.5, -0.5], [1.5, 0.3], [0.5 / 7, 0.5 / 5]])
    coords = coords[None].repeat(2, 1, 1)
    out = Fn.point_sample(rows, coords)
    assert out.shape == (2, 7)
    assert torch.allclose(out[:, 0], rows[:, 0, 0] / 4) and torch.allclose(out[:, 2], rows[:, -1, -1] / 4)
    assert torch.allclose(out[:, 1], rows[:, -1, -1] / 4, atol=1e-5) and torch.allclose(out[:, 3], rows[:, -1, 0] / 4, atol=1e-5)
    assert torch.equal(out[:, 4], torch.zeros(2)) and torch.equal(out[:, 5], torch.zeros(2))      # all four taps outside
    assert torch.allclose(out[:, 6], rows[:, 0, 0])                                                 # a pixel centre


def test_byte_targets_equal_float_targets_bit_for_bit():
    g = torch.Generator().manual_seed(4)
    pred, tgt = torch.randn(6, 2, 9, 11, generator=g), torch.rand(3, 2, 18, 22, generator=g) > 0.5      # targets at their own size
    coords, logits, ids = torch.rand(1, 70, 2, generator=g), torch.randn(6, 5, generator=g), torch.tensor([0, 3, 4])
    base = Fn.match_cost(pred, tgt.float(), coords, logits, ids, 2, 5, 5)
    for t in (tgt, tgt.to(torch.uint8)):
        assert torch.equal(Fn.match_cost(pred, t, coords, logits, ids, 2, 5, 5), base)
    src, c2 = torch.randn(3, 9, 11, generator=g), torch.rand(3, 33, 2, generator=g)
    ref = Fn.point_mask_losses(src, tgt[:, 0].float(), c2, 2.0)
    for t in (tgt[:, 0], tgt[:, 0].to(torch.uint8)):
        got = Fn.point_mask_losses(src, t, c2, 2.0)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert torch.equal(Fn.point_sample(tgt[:, 0], c2), Fn.point_sample(tgt[:, 0].float(), c2))


def test_cpu_formulations_against_the_reference_sequence_in_fp64():
    g = torch.Generator().manual_seed(5)
    pred, tgt = torch.randn(9, 2, 13, 17, generator=g) * 3, (torch.rand(4, 2, 13, 17, generator=g) > 0.6).float()
    coords, logits, ids = torch.rand(1, 257, 2, generator=g), torch.randn(9, 6, generator=g), torch.tensor([0, 5, 2, 2])
    got = cpu_ops.match_cost_terms(pred, tgt, coords[0], logits, ids)
    for a, b in zip(got, cost_terms_torch(pred, tgt, coords, logits, ids, torch.float64)):
        assert (a.double() - b).abs().max() <= TOL
    src = pred[:4, 0].clone().requires_grad_(True)
    c2 = torch.rand(4, 100, 2, generator=g)
    lm, ld = Fn.point_mask_losses(src, tgt[:, 0], c2, 3.0)
    (5 * lm + 5 * ld).backward()
    s64 = pred[:4, 0].double().requires_grad_(True)
    rm, rd = point_losses_torch(s64, tgt[:, 0], c2, 3.0, torch.float64)
    (5 * rm + 5 * rd).backward()
    assert abs(float(lm) - float(rm)) <= TOL and abs(float(ld) - float(rd)) <= TOL
    assert (src.grad.double() - s64.grad).abs().max() <= 1e-6 * float(s64.grad.abs().max())


@pytest.mark.parametrize("Q,G", [(7, 3), (5, 5), (3, 7), (6, 0), (1, 1)])
def test_assignment_equals_scipy(Q, G):
    from scipy.optimize import linear_sum_assignment as scipy_lsa
    rng = np.random.RandomState(10 * Q + G)
    for tied in (False, True):
        C = rng.rand(Q, G).astype(np.float32)
        if tied:
            C = np.round(C * 3) / 3
        r, c = linear_sum_assignment(torch.from_numpy(C))
        rs, cs = scipy_lsa(C.astype(np.float64)) if G else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        assert r.dtype == c.dtype == np.int64
        assert np.array_equal(r, rs) and np.array_equal(c, cs), (Q, G, tied)


def test_matcher_with_no_targets_and_square_case():
    g = torch.Generator().manual_seed(6)
    m = VideoHungarianMatcher(2.0, 5.0, 5.0, num_points=32)
    out = {"pred_logits": torch.randn(2, 4, 6, generator=g), "pred_masks": torch.randn(2, 4, 2, 8, 8, generator=g)}
    tg = [{"labels": torch.zeros(0, dtype=torch.int64), "masks": torch.zeros(0, 2, 8, 8, dtype=torch.bool)},
          {"labels": torch.tensor([1, 2, 3, 0]), "masks": torch.rand(4, 2, 8, 8, generator=g) > 0.5}]
    idx = m(out, tg)
    assert idx[0][0].numel() == idx[0][1].numel() == 0 and idx[0][0].dtype == torch.int64
    assert torch.equal(idx[1][0], torch.arange(4)) and sorted(idx[1][1].tolist()) == [0, 1, 2, 3]
    crit = VideoSetCriterion(5, m, {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}, 0.1, ["labels", "masks"], 32, 3.0, 0.75)
    losses = crit({k: v[:1] for k, v in out.items()}, tg[:1])      # R = 0: the mask losses are zero, not an error
    assert float(losses["loss_mask"]) == 0.0 and float(losses["loss_dice"]) == 0.0 and float(losses["loss_ce"]) > 0


def test_half_predictions_are_upcast_before_sampling():
    g = torch.Generator().manual_seed(7)
    src = (torch.randn(2, 8, 9, generator=g) * 3).to(torch.bfloat16).requires_grad_(True)
    tgt, coords = torch.rand(2, 8, 9, generator=g) > 0.5, torch.rand(2, 40, 2, generator=g)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        lm, ld = Fn.point_mask_losses(src, tgt, coords, 1.0)
    ref = Fn.point_mask_losses(src.detach().float(), tgt, coords, 1.0)
    assert lm.dtype == torch.float32 and torch.equal(lm.detach(), ref[0]) and torch.equal(ld.detach(), ref[1])
    (lm + ld).backward()
    assert src.grad.dtype == torch.bfloat16 and float(src.grad.float().abs().sum()) > 0


def test_build_criterion_against_the_reference_from_config():
    from dvis_plus_amd.config import get_default_cfg
    rec = json.load(open(os.path.join(GOLDEN, "criterion_weight_dicts.json")))
    assert sorted(rec) == ["DVIS_Plus_Offline_R50", "DVIS_Plus_Offline_VitAdapterL", "DVIS_Plus_Online_R50", "MinVIS_R50"]
    for name, r in rec.items():
        cfg = get_default_cfg().merge(json.load(open(os.path.join(GOLDEN, f"cfg_{name}.json"))))
        crit = build_criterion(cfg)
        assert type(crit).__name__ == r["criterion"] and type(crit.matcher).__name__ == r["matcher"]
        assert crit.weight_dict == r["weight_dict"]
        assert [crit.matcher.cost_class, crit.matcher.cost_mask, crit.matcher.cost_dice] == r["cost"]
        assert crit.matcher.num_points == r["matcher_num_points"] and getattr(crit.matcher, "frames", None) == r["matcher_frames"]
        assert (crit.num_classes, crit.eos_coef, crit.losses, crit.num_points, crit.oversample_ratio,
                crit.importance_sample_ratio) == (r["num_classes"], r["eos_coef"], r["losses"], r["num_points"],
                                                  r["oversample_ratio"], r["importance_sample_ratio"])
    cfg = get_default_cfg().merge(json.load(open(os.path.join(GOLDEN, "cfg_MinVIS_R50.json"))))
    image = build_criterion(cfg, "MaskFormer")
    assert isinstance(image, SetCriterion) and isinstance(image.matcher, HungarianMatcher)
    with pytest.raises(ValueError):
        build_criterion(cfg, "NoSuchArch")


def test_models_still_drop_the_criterion():
    """Wiring a training forward is out of scope: from_config keeps returning criterion=None."""
    import inspect
    from dvis_plus_amd import meta_architecture as M
    assert "\"criterion\": None" in inspect.getsource(M)
