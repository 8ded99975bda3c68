"""The referring tracker's training step on the GPU: golden g15 with replayed draws (the reference's own training run), the
gradients against a CPU run of the same code, and an optimiser step followed by .eval() — the weight caches and captured graphs
must serve the new weights."""
import numpy as np
import pytest
import torch

from tracker_train_cases import G15, MODES, build_tracker, train_step

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-3, atol=1e-3)         # tests/test_golden_gpu.py, g4 tracker outputs: the contract ...
TIGHT = dict(rtol=2e-4, atol=5e-5)       # ... and its regression guard


@pytest.fixture(scope="module")
def g15():
    return G15()


@pytest.mark.parametrize("mode", MODES)
def test_training_step_vs_reference_and_vs_cpu(g15, mode):
    trk, out, indices, noised, losses = train_step(g15, mode, "cuda")
    assert np.array_equal(np.stack([np.asarray(i, dtype=np.int64) for i in indices]), g15.z[f"{mode}/indices"])
    for tol in (TOL, TIGHT):
        for k in ("pred_logits", "pred_masks", "pred_embds", "pred_references"):
            torch.testing.assert_close(out[k].detach().cpu(), g15.t(f"{mode}/{k}"), **tol)
        for i, a in enumerate(out["aux_outputs"]):
            for k in a:
                torch.testing.assert_close(a[k].detach().cpu(), g15.t(f"{mode}/aux{i}/{k}"), **tol)
        for k, v in losses.items():
            torch.testing.assert_close(v.detach().cpu(), g15.t(f"{mode}/loss/{k}"), **tol)
        for n, p in trk.named_parameters():
            torch.testing.assert_close(p.grad.cpu(), g15.grads(mode)[n], **tol, msg=lambda m, n=n: f"{n}: {m}")
    # against the CPU run of the same code: 4 x the error of the fp32 CPU run against the fp64 CPU run, per parameter
    cpu32 = dict(train_step(g15, mode, "cpu")[0].named_parameters())
    cpu64 = dict(train_step(g15, mode, "cpu", torch.float64)[0].named_parameters())
    base = cpu_baselines(cpu32, cpu64)
    for n, p in trk.named_parameters():
        bound = 4 * base[n]
        err = (p.grad.cpu().double() - cpu64[n].grad).abs().max().item()
        print(f"{mode} {n}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (n, err, bound)


MIN_SAMPLES = 64


def cpu_baselines(cpu32, cpu64):
    """{parameter: max |fp32 CPU gradient - fp64 CPU gradient|}, the figure the GPU gradient gets 4 x of.

    The figure is a maximum over the parameter's elements, so it is only as steady as the parameter is large.  class_embed.bias
    has classes + 1 = 6 elements: on the same inputs two CPU hosts gave 3.2e-08 and 1.2e-07 for it (rs; 0.5 and 2 ulp of its
    largest gradient, 0.64), while every parameter of 64 elements or more agreed within 1.3 x (class_embed.weight: 4.705e-07 and
    4.703e-07).  Four times the luckier figure is below what a correctly working fp32 run gives (the device's: 1.7e-07, a path
    of torch ops alone).  So a parameter of fewer than MIN_SAMPLES elements takes the relative error of the large parameters of
    its own module, which contract the same upstream gradient, at its own scale, where that is larger than its own figure."""
    err = {n: (cpu32[n].grad.double() - cpu64[n].grad).abs().max().item() for n in cpu64}
    scale = {n: cpu64[n].grad.abs().max().item() for n in cpu64}
    out = {}
    for n in cpu64:
        out[n] = err[n]
        if cpu64[n].numel() < MIN_SAMPLES:
            module = n.rsplit(".", 1)[0]
            rel = [err[m] / scale[m] for m in cpu64 if m.rsplit(".", 1)[0] == module and cpu64[m].numel() >= MIN_SAMPLES]
            if rel:
                out[n] = max(err[n], max(rel) * scale[n])
    return out


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("graphs", [True, False])
def test_eval_after_an_optimiser_step_serves_the_new_weights(g15, graphs, fused):
    fe, fn, mf = (g15.t(k).cuda() for k in ("in/frame_embeds", "in/frame_embeds_no_norm", "in/mask_features"))

    def evaluate(trk):
        trk.eval()
        trk.use_graphs, trk.fused_chain = graphs, fused
        with torch.no_grad():
            a = trk(fe[:, :, :2], mf[:, :2], frame_embeds_no_norm=fn[:, :, :2])
            b = trk(fe[:, :, 2:], mf[:, 2:], resume=True, frame_embeds_no_norm=fn[:, :, 2:])
        return [x[k].clone() for x in (a, b) for k in ("pred_logits", "pred_masks", "pred_embds", "pred_references")]
    trk = build_tracker(g15, "none", "cuda")
    before = evaluate(trk)                          # fills the K/V, Q, out-projection caches and captures the graphs
    trk.train()
    opt = torch.optim.SGD(trk.parameters(), lr=0.05)
    out = trk(fe, mf, frame_embeds_no_norm=fn)
    (out["pred_masks"].square().mean() + out["pred_logits"].square().mean()
     + sum(a["pred_masks"].square().mean() for a in out["aux_outputs"])).backward()
    assert all(p.grad is not None for p in trk.parameters())
    opt.step()
    after = evaluate(trk)
    fresh = build_tracker(g15, "none", "cuda")
    fresh.load_state_dict(trk.state_dict(), strict=True)
    want = evaluate(fresh)
    assert any(not torch.equal(x, y) for x, y in zip(before, after)), "the step changed nothing"
    for x, y in zip(after, want):
        assert torch.equal(x, y)


def test_online_model_training_forward():
    """DVIS_Plus_online in .train() on the toy backbone with duck-typed instances: loss keys = the weight_dict's (with the
    contrastive key), finite, gradients for every tracker parameter and no segmenter parameter, iter advances, the second call
    (iter >= max_iter_num // 2) matches on the tracker's own outputs."""
    from tracker_train_cases import check_online_training
    check_online_training("cuda")


def test_online_model_eval_after_a_training_call():
    """Eval on the same video after a training call = a model that never trained, bit for bit; weights unchanged."""
    from tracker_train_cases import check_eval_after_training
    check_eval_after_training("cuda")
