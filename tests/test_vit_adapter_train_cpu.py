"""ViT-Adapter training on the CPU (host logic): golden g19 — the reference's own DinoV2ViTAdapter in .train() with a frozen ViT —
against this package's module: outputs, gradients, BatchNorm buffers; the frozen ViT's flags; the finetune refusal; the cfg keys;
eval after an optimiser step."""
import pytest
import torch

from vit_adapter_train_cases import G19, OUTS, build_adapter, g19_loss, is_bn_buffer

TOL = dict(rtol=1e-3, atol=1e-3)         # tests/test_tracker_train_gpu.py: the contract ...
TIGHT = dict(rtol=2e-4, atol=5e-5)       # ... and its regression guard


@pytest.fixture(scope="module")
def g19():
    return G19()


def test_fixture_conditions_are_recorded(g19):
    m = g19.meta
    assert m["smallest_distance_to_integer"] >= m["margin"] == 5e-5 and m["largest_fp32_fp64_coordinate_diff"] <= m["margin"] / 10
    assert m["smallest_relu_margin_in_own_differences"] >= 10 and m["smallest_pool_gap_in_own_differences"] >= 10
    assert m["frames"] in (2, 3) and m["coordinates"] > 0 and m["relu_pre_activations"] > 0 and m["pool_windows"] > 0


def test_g19_training_step_vs_reference(g19):
    m, outs, grads, bufs = g19.run("cpu")
    assert set(grads) == set(g19.grads) and set(bufs) == set(g19.buffers)
    for tol in (TOL, TIGHT):
        for k in OUTS:
            torch.testing.assert_close(outs[k], g19.outs[k], **tol, msg=lambda s, k=k: f"{k}: {s}")
        for n, g in grads.items():
            torch.testing.assert_close(g, g19.grads[n], **tol, msg=lambda s, n=n: f"{n}: {s}")
        for n, b in bufs.items():
            torch.testing.assert_close(b, g19.buffers[n], **tol, msg=lambda s, n=n: f"{n}: {s}")
    # the step moved the running statistics (momentum 0.1) and counted one batch
    moved = [n for n in bufs if not n.endswith("num_batches_tracked") and not torch.equal(bufs[n], g19.state[n])]
    assert len(moved) == sum(not n.endswith("num_batches_tracked") for n in bufs)
    assert all(int(b) == int(g19.state[n]) + 1 for n, b in bufs.items() if n.endswith("num_batches_tracked"))


def test_the_frozen_vit_gets_no_gradient(g19):
    m, _, grads, _ = g19.run("cpu")
    vit = dict(m.vit_module.named_parameters())
    assert vit and all(not p.requires_grad and p.grad is None for p in vit.values())
    rest = {n: p for n, p in m.named_parameters() if not n.startswith("vit_module.")}
    assert set(rest) == set(grads) and all(p.requires_grad and p.grad is not None and torch.isfinite(p.grad).all() for p in rest.values())
    assert m.level_embed.grad is not None and float(m.level_embed.grad.abs().max()) > 0
    # not frozen by flag: the ViT still runs under no_grad (adapter.py:540-544, :288-293) and still gets no gradient
    m = build_adapter(g19.meta["cfg"], state=g19.state, freeze_backbone=False).train()
    assert all(p.requires_grad for p in m.vit_module.parameters())
    g19_loss(m(g19.x), g19.cots).backward()
    assert all(p.grad is None for p in m.vit_module.parameters()) and m.spm.fc1.weight.grad is not None


def test_with_cp_changes_nothing(g19):
    a = build_adapter(g19.meta["cfg"], state=g19.state, with_cp=True).train()
    b = build_adapter(g19.meta["cfg"], state=g19.state, with_cp=False).train()
    assert a.with_cp and not b.with_cp
    assert all(torch.equal(p, q) for p, q in zip(a(g19.x), b(g19.x)))


def test_finetune_is_refused(g19):
    with pytest.raises(NotImplementedError, match="self-attention backward"):
        build_adapter(g19.meta["cfg"], finetune=True)
    from dvis_plus_amd.config import get_default_cfg
    from dvis_plus_amd.vit_adapter import D2VitAdapterDinoV2
    cfg = get_default_cfg()
    cfg.MODEL.VIT_ADAPTER.NAME = "vitb"
    cfg.MODEL.VIT_ADAPTER.FINETUNE = True
    with pytest.raises(NotImplementedError, match="FINETUNE"):
        D2VitAdapterDinoV2(cfg, None)


def test_cfg_keys_are_read(monkeypatch):
    """D2VitAdapterDinoV2(cfg, ...) hands MODEL.VIT_ADAPTER.{FREEZE_VIT, FINETUNE, FINETUNE_INDEXES, WITH_CP} to the constructor
    (the constructor itself is exercised above; here it is replaced so that no ViT-B is built)."""
    from dvis_plus_amd import vit_adapter as VA
    from dvis_plus_amd.config import get_default_cfg
    seen = {}
    monkeypatch.setattr(VA, "get_adapter_args", lambda name: {"size": name})
    monkeypatch.setattr(VA.DinoV2ViTAdapter, "__init__", lambda self, **kw: (torch.nn.Module.__init__(self), seen.update(kw))[0])
    cfg = get_default_cfg()
    cfg.MODEL.VIT_ADAPTER.merge({"NAME": "vitb", "FREEZE_VIT": True, "FINETUNE": False, "FINETUNE_INDEXES": [1, 3], "WITH_CP": True})
    VA.D2VitAdapterDinoV2(cfg, None)
    assert seen == dict(size="vitb", freeze_backbone=True, finetune=False, finetune_indexes=[1, 3], with_cp=True)
    cfg.MODEL.VIT_ADAPTER.FREEZE_VIT = False
    seen.clear()
    VA.D2VitAdapterDinoV2(cfg, None)
    assert seen["freeze_backbone"] is False
    seen.clear()
    VA.D2VitAdapterDinoV2("vitl")                     # by size name: the constructor's defaults
    assert seen == dict(size="vitl")


def test_eval_after_a_step_equals_a_fresh_model_with_the_same_state(g19):
    def evaluate(m):
        m.eval()
        with torch.no_grad():
            return [f.clone() for f in m(g19.x)]
    m = build_adapter(g19.meta["cfg"], state=g19.state)
    before = evaluate(m)                         # fills the derived tensors (LayerScale folds, flat patch weights, BatchNorm affines)
    m.train()
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1.0)       # (gradients of about 1e-3: a small, sane step)
    g19_loss(m(g19.x), g19.cots).backward()
    opt.step()
    after = evaluate(m)
    assert all(not torch.equal(a, b) for a, b in zip(after, before))
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert all(torch.equal(state[k], g19.state[k]) for k in state if k.startswith("vit_module."))
    assert any(not torch.equal(state[k], g19.state[k]) for k in state if is_bn_buffer(k))
    fresh = build_adapter(g19.meta["cfg"], state=state)
    assert all(torch.equal(a, b) for a, b in zip(after, evaluate(fresh)))
