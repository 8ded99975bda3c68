"""The masked-attention decoder's training step on the GPU: golden g17 (the reference's own training run) — the forward kernels,
csrc/masked_attention_backward.hip in the cross-attentions (18, 72 and 288 keys), csrc/attention_backward.hip in the
self-attentions, the mask logits' backward kernels — the gradients against the fp64 CPU run of the same code, and an optimiser step
followed by .eval(): the weight caches must serve the new weights."""
import pytest
import torch

from decoder_train_cases import G17, build_decoder, check_predictions, golden_grads, train_run
from test_tracker_train_gpu import MIN_SAMPLES, TIGHT, TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g17():
    return G17()


@pytest.fixture(scope="module")
def cpu_runs(g17):
    """The fp32 and fp64 CPU gradients, computed once and left unchanged."""
    return train_run(g17, "cpu")[3], train_run(g17, "cpu", torch.float64)[3]


def _baselines(cpu32, cpu64):
    """tests/test_refiner_train_gpu.py's scheme: {tensor: max |fp32 CPU - fp64 CPU|}; a parameter of fewer than MIN_SAMPLES elements
    takes the relative error of the large parameters of its own module at its own scale, where that is larger than its own figure."""
    err = {n: (cpu32[n].double() - cpu64[n]).abs().max().item() for n in cpu64}
    scale = {n: cpu64[n].abs().max().item() for n in cpu64}
    out = {}
    for n in cpu64:
        out[n] = err[n]
        if cpu64[n].numel() < MIN_SAMPLES:
            module = n.rsplit(".", 1)[0]
            rel = [err[m] / scale[m] for m in cpu64 if m.rsplit(".", 1)[0] == module and cpu64[m].numel() >= MIN_SAMPLES]
            if rel:
                out[n] = max(err[n], max(rel) * scale[n])
    return out


@pytest.mark.parametrize("features_grad", [True, False])
def test_training_step_vs_reference_and_vs_cpu(g17, cpu_runs, features_grad):
    """features_grad: mask_features requires grad — one Fn.mask_logits call per prediction, the features' gradient from the forward
    kernel on transposed operands; without it ONE call with (L + 1) Q rows per frame."""
    dec, out, masks, grads = train_run(g17, "cuda", features_grad=features_grad)
    for i, (got, want) in enumerate(zip(masks, g17.masks())):
        assert torch.equal(got.cpu(), want), f"layer {i}: effective attention mask differs from the recording"
    assert len(masks) == g17.meta["layers"] == len(out["aux_outputs"])
    check_predictions(g17, out, (TOL, TIGHT))
    want = golden_grads(g17)
    assert set(grads) == set(want) - (set() if features_grad else {"mask_features"})
    for tol in (TOL, TIGHT):
        for n, g in grads.items():
            torch.testing.assert_close(g.cpu(), want[n], **tol, msg=lambda m, n=n: f"{n}: {m}")
    cpu32, cpu64 = cpu_runs
    base = _baselines(cpu32, cpu64)
    worst = 0.0
    for n, g in grads.items():
        err = (g.cpu().double() - cpu64[n]).abs().max().item()
        worst = max(worst, err / base[n])
        print(f"{n}: err {err:.3e} bound {4 * base[n]:.3e}")
    print(f"worst ratio to the fp32 CPU error: {worst:.2f}")
    for n, g in grads.items():
        err = (g.cpu().double() - cpu64[n]).abs().max().item()
        assert err <= 4 * base[n], (n, err, 4 * base[n])


def test_eval_after_an_optimiser_step_serves_the_new_weights(g17):
    from dvis_plus_amd import functions as Fn
    from decoder_train_cases import loss_of
    assert Fn.x3_on()
    x, mf = g17.inputs("cuda")
    keys = ("pred_logits", "pred_masks", "pred_embds", "pred_embds_without_norm", "pred_reid_embed")

    def evaluate(dec):
        dec.eval()
        with torch.no_grad():
            out = dec(x, mf)
        assert out["aux_outputs"] == []
        return [out[k].clone() for k in keys]
    dec = build_decoder(g17, "cuda")
    before = evaluate(dec)                                   # fills the per-level K / V weight cache
    dec.train()
    opt = torch.optim.SGD(dec.parameters(), lr=0.5)
    loss_of(dec(x, mf), g17.cot("cuda"), g17.meta["hidden"]).mul(1e3).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in dec.parameters())
    opt.step()
    after = evaluate(dec)
    assert all(not torch.equal(a, b) for a, b in zip(after, before))
    fresh = build_decoder(g17, "cuda", state={k: v.detach().cpu() for k, v in dec.state_dict().items()})
    assert all(torch.equal(a, b) for a, b in zip(after, evaluate(fresh)))
