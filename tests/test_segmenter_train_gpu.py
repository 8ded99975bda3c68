"""Segmenter training on the GPU: golden g18 (the reference's own pixel decoder in .train()) through `_train_features` with
Fn.msda_fused in the encoder layers, an optimiser step followed by .eval() (the weight caches must serve the new weights), and the
MinVIS stage against its fp64 CPU run."""
import pytest
import torch

from segmenter_train_cases import G18, baselines, g18_loss, minvis_batch, minvis_model, spy_matcher
from test_tracker_train_gpu import TIGHT, TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def g18():
    return G18()


@pytest.fixture(scope="module")
def cpu_runs(g18):
    """The fp32 and fp64 CPU gradients, computed once and left unchanged."""
    return g18.run("cpu")[2], g18.run("cpu", torch.float64)[2]


def test_g18_training_step_vs_reference_and_vs_cpu(g18, cpu_runs, monkeypatch):
    from dvis_plus_amd import functions as Fn
    calls, inner = [], Fn.msda_fused_backward
    monkeypatch.setattr(Fn, "msda_fused_backward", lambda *a, **k: calls.append(1) or inner(*a, **k))
    pd, outs, grads = g18.run(DEV)
    assert len(calls) == g18.meta["layers"] == 2, "the fused op did not run in every encoder layer"
    want = g18.golden_grads()
    assert set(grads) == set(want)
    for tol in (TOL, TIGHT):
        for n, v in outs.items():
            torch.testing.assert_close(v.cpu(), g18.outs[n], **tol, msg=lambda m, n=n: f"{n}: {m}")
        for n, g in grads.items():
            torch.testing.assert_close(g.cpu(), want[n], **tol, msg=lambda m, n=n: f"{n}: {m}")
    cpu32, cpu64 = cpu_runs
    base = baselines(cpu32, cpu64)
    errs = {n: (g.cpu().double() - cpu64[n]).abs().max().item() for n, g in grads.items()}
    for n in grads:
        print(f"{n}: err {errs[n]:.3e} bound {4 * base[n]:.3e}")
    print(f"worst ratio to the fp32 CPU error: {max(errs[n] / base[n] for n in grads):.2f}")
    for n in grads:
        assert errs[n] <= 4 * base[n], (n, errs[n], 4 * base[n])


def test_eval_after_an_optimiser_step_serves_the_new_weights(g18):
    from dvis_plus_amd import functions as Fn
    from segmenter_train_cases import build_pixel_decoder
    assert Fn.x3_on()
    feats = {k: v.to(DEV) for k, v in g18.feats.items()}
    cot = {k: v.to(DEV) for k, v in g18.cots.items()}

    def evaluate(pd):
        pd.eval()
        with torch.no_grad():
            mf, _, ms = pd.forward_features(feats)
        return [mf.clone()] + [m.clone() for m in ms]
    pd = build_pixel_decoder(g18.meta, DEV, state=g18.state)
    before = evaluate(pd)                 # fills the caches: the fused offsets | logits projection, the split-f16 packs, the GN folds
    pd.train()
    opt = torch.optim.SGD(pd.parameters(), lr=0.5)
    mf, _, ms = pd.forward_features(feats)
    g18_loss(mf, ms, cot).mul(1e2).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in pd.parameters())
    opt.step()
    after = evaluate(pd)
    assert all(not torch.equal(a, b) for a, b in zip(after, before))
    fresh = build_pixel_decoder(g18.meta, DEV, state={k: v.detach().cpu() for k, v in pd.state_dict().items()})
    assert all(torch.equal(a, b) for a, b in zip(after, evaluate(fresh)))


def _seeded_draws(model, seed):
    """Every random draw of the criterion and its matcher from ONE seeded CPU generator: the same points on every device."""
    g = torch.Generator().manual_seed(seed)
    draw = lambda shape, device: torch.rand(shape, generator=g).to(device)
    model.criterion._rand = draw
    model.criterion.matcher._rand = draw


def _train_call(device, dtype=torch.float32):
    m, wd = minvis_model(device, dtype)
    _seeded_draws(m, 33)
    calls = spy_matcher(m)
    m.train()
    losses = m(minvis_batch(device))
    return m, wd, losses, calls


def test_minvis_stage_vs_the_fp64_cpu_run():
    m, wd, losses, calls = _train_call(DEV)
    assert set(losses) == set(wd) and all(torch.isfinite(v).all() for v in losses.values())
    _, _, want, calls64 = _train_call("cpu", torch.float64)
    assert len(calls) == len(calls64) > 0
    for a, b in zip(calls, calls64):
        assert all(torch.equal(r1, r2) and torch.equal(c1, c2) for (r1, c1), (r2, c2) in zip(a, b)), "the matcher's pairs differ"
    for k in wd:
        got, ref = losses[k].detach().cpu().double(), want[k].detach().double()      # (the criterion itself computes in float32)
        print(f"{k}: {float(got):.6f} vs fp64 CPU {float(ref):.6f}")
        torch.testing.assert_close(got, ref, **TOL, msg=lambda s, k=k: f"{k}: {s}")
    sum(losses.values()).backward()
    for name, mod in (("backbone", m.backbone), ("pixel_decoder", m.sem_seg_head.pixel_decoder), ("decoder", m.sem_seg_head.predictor)):
        for n, p in mod.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), (name, n)


def test_tracker_stage_on_a_shared_segmenter_leaves_it_frozen():
    """The same backbone and head first train as a MinVIS stage, then serve a DVIS_Plus_online.train() call: that call puts the
    segmenter back into .eval() and gives it no gradient."""
    from tracker_train_cases import online_model
    from dvis_plus_amd.criterion import VideoSetCriterion
    from dvis_plus_amd.matcher import VideoHungarianMatcher
    from dvis_plus_amd.meta_architecture import MinVIS
    online, video, _ = online_model(DEV)
    wd = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    matcher = VideoHungarianMatcher(num_points=64, cost_class=2.0, cost_mask=5.0, cost_dice=5.0)
    crit = VideoSetCriterion(online.sem_seg_head.num_classes, matcher=matcher, weight_dict=wd, eos_coef=0.1, losses=["labels", "masks"],
                             num_points=64, oversample_ratio=3.0, importance_sample_ratio=0.75).to(DEV)
    seg = MinVIS(backbone=online.backbone, sem_seg_head=online.sem_seg_head, num_queries=online.num_queries, criterion=crit,
                 num_frames=len(video["image"])).to(DEV).train()
    losses = seg([video])
    assert set(losses) == set(wd)
    sum(losses.values()).backward()
    shared = [p for mod in (online.backbone, online.sem_seg_head.pixel_decoder) for p in mod.parameters()]
    assert online.backbone.training and all(p.grad is not None for p in shared)
    seg.zero_grad(set_to_none=True)
    online.train()
    sum(online([video]).values()).backward()
    assert not online.backbone.training and not online.sem_seg_head.training and online.tracker.training
    assert all(p.grad is None for mod in (online.backbone, online.sem_seg_head) for p in mod.parameters())
    assert all(p.grad is not None for p in online.tracker.parameters())
