"""ViT-Adapter training on the GPU: golden g19 (the reference's own DinoV2ViTAdapter in .train(), frozen ViT) through
`DinoV2ViTAdapter._forward_train` with the ConvFFN's token-major convolution and the fused MSDeformAttn op on their own forward and
backward kernels, the same step with DVIS_DWCONV_TOKENS=0 (the reference's composition), and the MinVIS stage with this backbone
against its fp64 CPU run."""
import pytest
import torch

from segmenter_train_cases import baselines, minvis_batch, spy_matcher
from test_segmenter_train_gpu import _seeded_draws
from test_tracker_train_gpu import TOL
from vit_adapter_train_cases import G19, OUTS, minvis_vit_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def g19():
    return G19()


@pytest.fixture(scope="module")
def cpu_runs(g19):
    """The fp32 and fp64 CPU runs (outputs and gradients in one dict each), computed once and left unchanged."""
    def one(dtype):
        _, outs, grads, _ = g19.run("cpu", dtype)
        return {**{f"out.{k}": v for k, v in outs.items()}, **grads}
    return one(torch.float32), one(torch.float64)


def _gpu_step(g19, monkeypatch, kernel=True):
    from dvis_plus_amd import functions as Fn
    calls = {"dwconv": 0, "msda": 0}
    dw, ms = Fn.dwconv3x3_tokens_backward, Fn.msda_fused_backward
    monkeypatch.setattr(Fn, "dwconv3x3_tokens_backward", lambda *a, **k: (calls.__setitem__("dwconv", calls["dwconv"] + 1), dw(*a, **k))[1])
    monkeypatch.setattr(Fn, "msda_fused_backward", lambda *a, **k: (calls.__setitem__("msda", calls["msda"] + 1), ms(*a, **k))[1])
    monkeypatch.setenv("DVIS_DWCONV_TOKENS", "1" if kernel else "0")
    m, outs, grads, bufs = g19.run(DEV)
    return m, outs, grads, bufs, calls


def _check_rule(got, cpu_runs, what):
    cpu32, cpu64 = cpu_runs
    base = baselines(cpu32, cpu64)
    assert set(got) == set(cpu64)
    errs = {n: (g.cpu().double() - cpu64[n]).abs().max().item() for n, g in got.items()}
    for n in got:
        print(f"{what} {n}: err {errs[n]:.3e} bound {4 * base[n]:.3e}")
    print(f"{what}: worst ratio to the fp32 CPU error: {max(errs[n] / base[n] for n in got):.2f}")
    bad = {n: (errs[n], 4 * base[n]) for n in got if not errs[n] <= 4 * base[n]}
    assert not bad, bad


def test_g19_training_step_vs_reference_and_vs_cpu(g19, cpu_runs, monkeypatch):
    m, outs, grads, bufs, calls = _gpu_step(g19, monkeypatch)
    assert calls == {"dwconv": 6, "msda": 6}, f"the six extractors did not run on the backward kernels: {calls}"
    assert set(grads) == set(g19.grads) and set(bufs) == set(g19.buffers)
    assert all(p.grad is None and not p.requires_grad for p in m.vit_module.parameters())
    for k in OUTS:
        torch.testing.assert_close(outs[k].cpu(), g19.outs[k], **TOL, msg=lambda s, k=k: f"{k}: {s}")
    for n, g in grads.items():
        torch.testing.assert_close(g.cpu(), g19.grads[n], **TOL, msg=lambda s, n=n: f"{n}: {s}")
    for n, b in bufs.items():
        torch.testing.assert_close(b.cpu(), g19.buffers[n], **TOL, msg=lambda s, n=n: f"{n}: {s}")
    _check_rule({**{f"out.{k}": v for k, v in outs.items()}, **grads}, cpu_runs, "kernel path")


def test_kernel_path_against_the_composition(g19, cpu_runs, monkeypatch):
    """DVIS_DWCONV_TOKENS=0: the extractors' ConvFFN takes the reference's composition under autograd; both paths keep the rule."""
    _, outs0, grads0, _, calls0 = _gpu_step(g19, monkeypatch, kernel=False)
    assert calls0 == {"dwconv": 0, "msda": 6}
    _check_rule({**{f"out.{k}": v for k, v in outs0.items()}, **grads0}, cpu_runs, "composition")
    _, outs1, grads1, _, calls1 = _gpu_step(g19, monkeypatch, kernel=True)
    assert calls1["dwconv"] == 6
    _check_rule({**{f"out.{k}": v for k, v in outs1.items()}, **grads1}, cpu_runs, "kernel path")
    print("largest |kernel path - composition| over the gradients:",
          max(float((grads1[n] - grads0[n]).abs().max()) for n in grads1))


def test_eval_after_an_optimiser_step_serves_the_new_weights(g19):
    from vit_adapter_train_cases import build_adapter, g19_loss
    x = g19.x.to(DEV)
    cot = {k: v.to(DEV) for k, v in g19.cots.items()}

    def evaluate(m):
        m.eval()
        with torch.no_grad():
            return [f.clone() for f in m(x)]
    m = build_adapter(g19.meta["cfg"], DEV, state=g19.state)
    before = evaluate(m)
    m.train()
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1.0)       # (gradients of about 1e-3: a small, sane step)
    g19_loss(m(x), cot).backward()
    opt.step()
    after = evaluate(m)
    assert all(torch.isfinite(a).all() for a in after)
    assert all(not torch.equal(a, b) for a, b in zip(after, before))
    fresh = build_adapter(g19.meta["cfg"], DEV, state={k: v.detach().cpu() for k, v in m.state_dict().items()})
    assert all(torch.equal(a, b) for a, b in zip(after, evaluate(fresh)))
    from dvis_plus_amd import functions as Fn
    Fn.X3_GUARD.check_now(x.device)              # no split-f16 kernel of these evaluations left its range


def _train_call(device, dtype=torch.float32):
    m, wd = minvis_vit_model(device, dtype)
    _seeded_draws(m, 33)
    calls = spy_matcher(m)
    m.train()
    losses = m(minvis_batch(device))
    return m, wd, losses, calls


def test_minvis_stage_with_this_backbone_vs_the_fp64_cpu_run():
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
    for n, p in m.backbone.named_parameters():
        if n.startswith("vit_module."):
            assert p.grad is None, n
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), ("backbone", n)
    for name, mod in (("pixel_decoder", m.sem_seg_head.pixel_decoder), ("decoder", m.sem_seg_head.predictor)):
        for n, p in mod.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), (name, n)
