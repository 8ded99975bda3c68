"""Set criterion on the GPU, through the C ABI of csrc/criterion.hip: the g14 comparisons of test_criterion_cpu.py on device
tensors, and at the production shape (Q = 100 / 200, G = 12, T = 5, 184 x 320, K = 12 544, seeded structured inputs) against an
fp64 torch evaluation of the reference's op sequence computed here on the CPU.

Bounds (set before any run, from the reference's own error): unweighted cost terms and the two losses max(1e-5, 8 e32) under the
project's hard ceiling 1e-3, e32 = the error of the fp32 torch formulation on the CPU against the same fp64 values; grad_src
max(4 e32_g, 1e-6 max|g64|); integer outputs (indices) exactly scipy's on the kernel's own C and equal to the fp64 evaluation's.
Every figure is printed before it is asserted (run with -s to see them)."""
import numpy as np
import pytest
import torch

from criterion_cases import G14, Replay, cost_terms_torch, point_losses_torch, structured

from dvis_plus_amd import functions as Fn
from dvis_plus_amd.criterion import SetCriterion, VideoSetCriterion
from dvis_plus_amd.matcher import (HungarianMatcher, VideoHungarianMatcher, VideoHungarianMatcher_Consistent,
                                   linear_sum_assignment)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
H, W, K, T, G = 184, 320, 12544, 5, 12
WEIGHTS = dict(cost_class=2.0, cost_mask=5.0, cost_dice=5.0)


@pytest.fixture(scope="module")
def g14():
    return G14()


def _matcher(g14, cls, **kw):
    return cls(num_points=g14.meta["K"], **g14.meta["weights"], **kw)


@pytest.mark.parametrize("case", ["video", "image"])
def test_g14_cost_terms_and_indices(g14, case):
    image = g14.meta["cases"][case]["image"]
    out, tg = g14.outputs(case, DEV, layers=1), g14.targets(case, DEV)
    w = g14.meta["weights"]
    for b, t in enumerate(tg):
        C, terms = Fn.match_cost(out["pred_masks"][b], t["masks"], g14.t(case, f"match_draw_{b}").to(DEV), out["pred_logits"][b],
                                 t["labels"], w["cost_class"], w["cost_mask"], w["cost_dice"], return_terms=True)
        assert C.is_cuda
        ref_terms, ref_C = g14.t(case, f"match_terms_{b}"), g14.t(case, f"match_C_{b}")
        assert terms.shape == ref_terms.shape and C.shape == ref_C.shape
        if C.numel():
            e = float((terms.cpu() - ref_terms).abs().max())
            print(f"g14 {case} b{b}: terms max|err| {e:.2e}, C max|err| {float((C.cpu() - ref_C).abs().max()):.2e}")
            assert e <= TOL and (C.cpu() - ref_C).abs().max() <= 12 * TOL
    m = _matcher(g14, HungarianMatcher if image else VideoHungarianMatcher)
    m._rand = Replay([g14.t(case, f"match_draw_{b}") for b in range(len(tg))])
    for b, (i, j) in enumerate(m(out, tg)):
        assert i.device.type == "cpu" and i.dtype == torch.int64
        assert np.array_equal(torch.stack((i, j)).numpy(), g14.t(case, f"match_idx_{b}").numpy()), (case, b)


def test_g14_consistent_matcher(g14):
    c = g14.meta["cases"]["consistent"]
    m = _matcher(g14, VideoHungarianMatcher_Consistent, frames=c["frames"])
    m._rand = Replay([g14.t("consistent", f"match_draw_{i}") for i in range(c["n_draws"])])
    for b, (i, j) in enumerate(m(g14.outputs("consistent", DEV), g14.targets("consistent", DEV))):
        assert np.array_equal(torch.stack((i, j)).numpy(), g14.t("consistent", f"match_idx_{b}").numpy())


@pytest.mark.parametrize("case", ["video", "image"])
def test_g14_criterion_losses_and_gradient(g14, case):
    c = g14.meta["cases"][case]
    wd = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    wd.update({f"{k}_{i}": v for i in range(c["n_aux"]) for k, v in list(wd.items())[:3]})
    kw = dict(weight_dict=wd, eos_coef=0.1, losses=["labels", "masks"], num_points=g14.meta["K"], oversample_ratio=3.0,
              importance_sample_ratio=0.75)
    crit = (SetCriterion(g14.meta["NCLS"], matcher=_matcher(g14, HungarianMatcher), **kw) if c["image"] else
            VideoSetCriterion(g14.meta["NCLS"], matcher=_matcher(g14, VideoHungarianMatcher), **kw)).to(DEV)
    replay = Replay([g14.t(case, f"crit_draw_{i:02d}") for i in range(c["n_crit_draws"])])
    crit._rand = crit.matcher._rand = replay
    out = g14.outputs(case, DEV, requires_grad=True)
    losses = crit(out, g14.targets(case, DEV))
    assert replay.i == c["n_crit_draws"] and sorted(losses) == c["loss_keys"]
    for k, v in losses.items():
        ref = float(g14.t(case, f"loss/{k}"))
        print(f"g14 {case} {k}: {float(v.detach()):.7f} ref {ref:.7f}")
        assert v.is_cuda and abs(float(v.detach()) - ref) <= TOL * max(1.0, abs(ref)), (k, float(v.detach()), ref)
    sum(losses[k] * wd[k] for k in losses).backward()
    g, ref = out["pred_masks"].grad.cpu(), g14.t(case, "grad_pred_masks")
    if c["image"]:
        ref = ref[:, :, 0]
    e = float((g - ref).abs().max())
    print(f"g14 {case} grad max|err| {e:.2e} of max {float(ref.abs().max()):.2e}")
    assert e <= 1e-6 * max(1.0, float(ref.abs().max())) + 1e-8


@pytest.fixture(scope="module")
def production():
    """Per Q: inputs, the fp64 evaluation and the fp32 CPU formulation's error against it (computed once)."""
    cache = {}

    def get(Q):
        if Q not in cache:
            pred, tgt, labels, logits, owners = structured(1000 + Q, Q, G, T, H, W)
            coords = torch.rand(1, K, 2, generator=torch.Generator().manual_seed(Q))
            t64 = cost_terms_torch(pred, tgt, coords, logits, labels, torch.float64)
            t32 = cost_terms_torch(pred, tgt, coords, logits, labels, torch.float32)
            e32 = [float((a.double() - b).abs().max()) for a, b in zip(t32, t64)]
            cache[Q] = dict(pred=pred, tgt=tgt, labels=labels, logits=logits, owners=owners, coords=coords, t64=t64, e32=e32)
        return cache[Q]
    return get


@pytest.mark.parametrize("Q", [100, 200])
def test_production_cost_terms_and_indices(production, Q):
    from scipy.optimize import linear_sum_assignment as scipy_lsa
    p = production(Q)
    args = (p["pred"].to(DEV), p["tgt"].to(DEV), p["coords"].to(DEV), p["logits"].to(DEV), p["labels"].to(DEV))
    C, terms = Fn.match_cost(*args, **WEIGHTS, return_terms=True)
    C2, terms2 = Fn.match_cost(*args, **WEIGHTS, return_terms=True)
    assert torch.equal(C, C2) and torch.equal(terms, terms2), "match_cost is not run-to-run identical"
    for name, got, ref, e32 in zip(("class", "mask", "dice"), terms.cpu(), p["t64"], p["e32"]):
        err = float((got.double() - ref).abs().max())
        bound = max(1e-5, 8 * e32)
        print(f"Q {Q} cost_{name}: max|err vs fp64| {err:.2e}  fp32-CPU e32 {e32:.2e}  bound {bound:.2e}  max|term| {float(ref.abs().max()):.3f}")
        assert bound <= 1e-3 and err <= bound, (name, err, bound)
    # float targets give the same bits as byte targets
    assert torch.equal(Fn.match_cost(args[0], args[1].float(), *args[2:], **WEIGHTS), C)
    r, c = linear_sum_assignment(C)
    rs, cs = scipy_lsa(C.cpu().numpy().astype(np.float64))
    assert np.array_equal(r, rs) and np.array_equal(c, cs), "indices differ from scipy's on the kernel's own C"
    C64 = 5.0 * p["t64"][1] + 2.0 * p["t64"][0] + 5.0 * p["t64"][2]
    r64, c64 = scipy_lsa(C64.numpy())
    assert np.array_equal(r, r64) and np.array_equal(c, c64), "indices differ from the fp64 evaluation's"
    assert sorted(r.tolist()) == sorted(p["owners"].tolist())


@pytest.fixture(scope="module")
def production_loss(production):
    p = production(100)
    order = p["owners"]
    src = p["pred"][order].flatten(0, 1).contiguous()                 # (60, H, W) matched rows
    tgt = p["tgt"].flatten(0, 1).contiguous()
    coords = torch.rand(src.shape[0], K, 2, generator=torch.Generator().manual_seed(77))
    nm = 12.0
    res = {}
    for dt in (torch.float64, torch.float32):
        s = src.clone().to(dt).requires_grad_(True)
        lm, ld = point_losses_torch(s, tgt, coords, nm, dt)
        (5.0 * lm + 5.0 * ld).backward()
        res[dt] = (float(lm.detach()), float(ld.detach()), s.grad)
    return dict(src=src, tgt=tgt, coords=coords, nm=nm, r64=res[torch.float64], r32=res[torch.float32])


def _run_losses(pl, deterministic=None):
    s = pl["src"].detach().to(DEV).requires_grad_(True)
    lm, ld = Fn.point_mask_losses(s, pl["tgt"].to(DEV), pl["coords"].to(DEV), pl["nm"], deterministic=deterministic)
    (5.0 * lm + 5.0 * ld).backward()
    return lm.detach(), ld.detach(), s.grad


def test_production_losses_and_gradient(production_loss):
    pl = production_loss
    lm, ld, g = _run_losses(pl)
    lm2, ld2, _ = _run_losses(pl)
    assert torch.equal(lm, lm2) and torch.equal(ld, ld2), "the loss forward is not run-to-run identical"
    for name, got, ref, r32 in (("loss_mask", float(lm), pl["r64"][0], pl["r32"][0]), ("loss_dice", float(ld), pl["r64"][1], pl["r32"][1])):
        e32 = abs(r32 - ref)
        bound = max(1e-5, 8 * e32)
        print(f"{name}: {got:.8f} fp64 {ref:.8f} |err| {abs(got - ref):.2e} e32 {e32:.2e} bound {bound:.2e}")
        assert bound <= 1e-3 and abs(got - ref) <= bound
    g64 = pl["r64"][2]
    e32g = float((pl["r32"][2].double() - g64).abs().max())
    bound = max(4 * e32g, 1e-6 * float(g64.abs().max()))
    err = float((g.cpu().double() - g64).abs().max())
    print(f"grad_src: max|g - g64| {err:.3e}  e32_g {e32g:.3e}  ratio {err / max(e32g, 1e-30):.2f}  max|g64| {float(g64.abs().max()):.3e}  bound {bound:.3e}")
    assert err <= bound
    # the reproducible form: the same bits twice, and within the same bound
    with_det = [_run_losses(pl, deterministic=True)[2] for _ in range(2)]
    assert torch.equal(with_det[0], with_det[1]), "the deterministic backward is not run-to-run identical"
    err = float((with_det[0].cpu().double() - g64).abs().max())
    print(f"grad_src (deterministic): max|g - g64| {err:.3e}  ratio {err / max(e32g, 1e-30):.2f}")
    assert err <= bound
    torch.use_deterministic_algorithms(True)
    try:
        g3 = _run_losses(pl)[2]
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(g3, with_det[0]), "torch.use_deterministic_algorithms(True) must select the reproducible backward"


def test_strict_mode_raises_for_unserved_dtypes(monkeypatch):
    g = torch.Generator().manual_seed(8)
    src = torch.randn(2, 8, 9, generator=g, dtype=torch.float64).to(DEV)
    tgt, coords = (torch.rand(2, 8, 9, generator=g) > 0.5).to(DEV), torch.rand(2, 30, 2, generator=g).to(DEV)
    monkeypatch.delenv("DVIS_STRICT", raising=False)
    with pytest.raises(RuntimeError, match="DVIS_STRICT"):
        Fn.point_mask_losses(src.requires_grad_(True), tgt, coords, 1.0)
    with pytest.raises(RuntimeError, match="DVIS_STRICT"):
        Fn.match_cost(src[:, None], tgt[:, None], coords[:1], torch.randn(2, 4, device=DEV), torch.tensor([0, 1], device=DEV))
    with pytest.raises(RuntimeError, match="DVIS_STRICT"):
        Fn.point_sample(src, coords)
    monkeypatch.setenv("DVIS_STRICT", "0")      # the explicit opt-out: the torch formulation, on the GPU
    lm, ld = Fn.point_mask_losses(src, tgt, coords, 1.0)
    ref = Fn.point_mask_losses(src.float(), tgt, coords, 1.0)
    assert abs(float(lm.detach()) - float(ref[0].detach())) <= TOL and abs(float(ld.detach()) - float(ref[1].detach())) <= TOL


def test_views_odd_point_counts_sizes_and_empty_rows():
    g = torch.Generator().manual_seed(9)
    big = torch.randn(2, 9, 3, 37, 60, generator=g) * 3
    view = big[1, :, :, :, 3:56]                                  # (9, 3, 37, 53): a non-contiguous view
    assert not view.is_contiguous()
    tgt = torch.rand(4, 3, 74, 106, generator=g) > 0.6            # targets at twice the size
    logits, ids = torch.randn(9, 7, generator=g), torch.tensor([6, 0, 3, 3])
    for k in (1, 63, 65, 257):                                    # K not a multiple of 64
        coords = torch.rand(1, k, 2, generator=g)
        coords[0, 0] = torch.tensor([0.0, 1.0])
        got = Fn.match_cost(view.to(DEV), tgt.to(DEV), coords.to(DEV), logits.to(DEV), ids.to(DEV), **WEIGHTS, return_terms=True)[1]
        ref = cost_terms_torch(view, tgt, coords, logits, ids, torch.float64)
        for a, b in zip(got.cpu(), ref):
            assert (a.double() - b).abs().max() <= TOL, k
    # 40 targets: more than one tile of 32
    tgt40 = torch.rand(40, 1, 20, 30, generator=g) > 0.5
    pred = torch.randn(70, 1, 20, 30, generator=g)
    coords, lg, id40 = torch.rand(1, 100, 2, generator=g), torch.randn(70, 5, generator=g), torch.randint(0, 5, (40,), generator=g)
    got = Fn.match_cost(pred.to(DEV), tgt40.to(DEV), coords.to(DEV), lg.to(DEV), id40.to(DEV), return_terms=True)[1]
    for a, b in zip(got.cpu(), cost_terms_torch(pred, tgt40, coords, lg, id40, torch.float64)):
        assert (a.double() - b).abs().max() <= TOL
    # point_sample on rows, borders included, bytes and floats
    rows, c2 = view[:, 0], torch.rand(9, 77, 2, generator=g) * 1.2 - 0.1
    ref = Fn.point_sample(rows, c2)
    assert (Fn.point_sample(rows.to(DEV), c2.to(DEV)).cpu() - ref).abs().max() <= TOL
    bt = tgt[:, 0]
    assert torch.equal(Fn.point_sample(bt.to(DEV), c2[:4].to(DEV)), Fn.point_sample(bt.float().to(DEV), c2[:4].to(DEV)))
    # losses on a strided view with P = 77, then R = 0
    src = rows[:4].to(DEV).requires_grad_(True)
    lm, ld = Fn.point_mask_losses(src, bt.to(DEV), c2[:4].to(DEV), 2.0)
    (lm + ld).backward()
    grads = {}
    for dt in (torch.float64, torch.float32):
        s = rows[:4].to(dt).clone().requires_grad_(True)
        rm, rd = point_losses_torch(s, bt, c2[:4], 2.0, dt)
        (rm + rd).backward()
        grads[dt] = s.grad.double()
        if dt == torch.float64:
            assert abs(float(lm) - float(rm)) <= TOL and abs(float(ld) - float(rd)) <= TOL
    g64 = grads[torch.float64]
    e32g = float((grads[torch.float32] - g64).abs().max())      # the same bound as at the production shape
    err = float((src.grad.cpu().double() - g64).abs().max())
    print(f"odd shapes grad_src: max|g - g64| {err:.3e}  e32_g {e32g:.3e}  max|g64| {float(g64.abs().max()):.3e}")
    assert err <= max(4 * e32g, 1e-6 * float(g64.abs().max()))
    empty = torch.zeros(0, 37, 53, device=DEV, requires_grad=True)
    lm, ld = Fn.point_mask_losses(empty, torch.zeros(0, 37, 53, dtype=torch.bool, device=DEV), torch.zeros(0, 77, 2, device=DEV), 1.0)
    (lm + ld).backward()
    assert float(lm) == 0.0 and float(ld) == 0.0 and empty.grad.shape == (0, 37, 53)
    assert Fn.point_sample(empty.detach(), torch.zeros(0, 5, 2, device=DEV)).shape == (0, 5)
