"""The refiner training stage on the GPU: the two g16 steps (attention forward kernel + csrc/attention_backward.hip, mask logits +
csrc/mask_gemm_backward.hip) against the reference's recording and against the fp64 CPU run of the same code, the inference
path after an optimiser step, and DVIS_Plus_offline in .train()."""
import pytest
import torch

from refiner_train_cases import (G16, STEPS, build_refiner, check_against_golden, check_offline_eval_after_training,
                                 check_offline_training, train_steps)
from test_tracker_train_gpu import MIN_SAMPLES, TIGHT, TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g16():
    return G16()


def _baselines(cpu32, cpu64):
    """test_tracker_train_gpu.cpu_baselines on dicts of gradients: {parameter: max |fp32 CPU - fp64 CPU|}; a parameter of fewer
    than MIN_SAMPLES elements takes the relative error of the large parameters of its own module at its own scale, where that is
    larger than its own figure (the reasons are written down there).

    One parameter has no scale of its own: `activation_proj.bias` shifts all T logits of a softmax over time by the same amount, so
    its exact gradient is 0 and what any fp32 run holds there is the rounding residue of sum_t a_t (g_t - sum a g) — terms that
    cancel.  Its fp64 figure is ~1e-17, the "relative error at its own scale" is therefore nothing, and its single fp32 CPU sample
    (of the order of 1e-9) is no baseline for a different summation order.  The residue is the rounding error of the SAME
    upstream gradient dz that `activation_proj.weight` contracts with the LayerNorm-ed queries (|x| = O(1)) and the bias with
    ones, so the bias takes the weight's ABSOLUTE fp32 CPU error where that is larger than its own."""
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
    out["activation_proj.bias"] = max(out["activation_proj.bias"], err["activation_proj.weight"])
    return out


def test_two_training_steps_vs_reference_and_vs_cpu(g16):
    ref, steps = train_steps(g16, "cuda")
    check_against_golden(g16, steps, (TOL, TIGHT))
    # against the CPU run of the same code: 4 x the error of the fp32 CPU run against the fp64 CPU run, per parameter.  Step 1
    # only: step 2 starts from weights that each run has updated with its own gradients.
    cpu32 = train_steps(g16, "cpu")[1][0]["grads"]
    cpu64 = train_steps(g16, "cpu", torch.float64)[1][0]["grads"]
    base = _baselines(cpu32, cpu64)
    worst = 0.0
    for n, grad in steps[0]["grads"].items():
        bound = 4 * base[n]
        err = (grad.cpu().double() - cpu64[n]).abs().max().item()
        worst = max(worst, err / base[n])
        print(f"{n}: err {err:.3e} bound {bound:.3e}")
    print(f"worst ratio to the fp32 CPU error: {worst:.2f}")
    for n, grad in steps[0]["grads"].items():
        err = (grad.cpu().double() - cpu64[n]).abs().max().item()
        assert err <= 4 * base[n], (n, err, 4 * base[n])


@pytest.mark.parametrize("graphs", [True, False])
def test_eval_after_an_optimiser_step_serves_the_new_weights(g16, graphs):
    ie, fe, mf = g16.inputs("cuda")

    def evaluate(ref):
        ref.eval()
        ref.use_graphs = graphs
        with torch.no_grad():
            out = ref(ie, fe, mf)
        return [out[k].clone() for k in ("pred_logits", "pred_masks", "pred_embds", "mask_embed")]
    ref = build_refiner(g16, "cuda")
    before = evaluate(ref)                          # fills the K/V and convolution caches and captures the graph
    ref.train()
    opt = torch.optim.SGD(ref.parameters(), lr=0.05)
    out = ref(ie, fe, mf)
    (out["pred_masks"].square().mean() + out["pred_logits"].square().mean() + out["pred_embds"].square().mean()
     + sum(a["pred_masks"].square().mean() + a["pred_logits"].square().mean() for a in out["aux_outputs"])).backward()
    assert all(p.grad is not None for p in ref.parameters())
    opt.step()
    after = evaluate(ref)
    fresh = build_refiner(g16, "cuda")
    fresh.load_state_dict(ref.state_dict(), strict=True)
    want = evaluate(fresh)
    assert all(not torch.equal(x, y) for x, y in zip(before, after)), "the step did not reach every output"
    for x, y in zip(after, want):
        assert torch.equal(x, y)


def test_offline_model_training_forward():
    check_offline_training("cuda")


def test_offline_model_eval_after_a_training_call():
    check_offline_eval_after_training("cuda")
