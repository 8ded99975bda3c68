"""CTVIS's segmenter stage on the GPU against g20 (the reference's own CTCLPlugin.train_loss and CTMinVIS.post_processing, recorded
draws replayed): integers equal, losses and the gradient to pred_reid_embed under the project's 4 x rule with the items on the
contrastive-items kernel, and CTMinVIS end to end at toy sizes."""
import pytest
import torch

import ctvis_cases as K
from dvis_plus_amd import functions as Fn
from segmenter_train_cases import minvis_batch
from test_ctvis_train_cpu import check_eval_on_g20_clip, eval_on_g20_clip

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def g20():
    return K.G20()


def count_kernel_calls(monkeypatch):
    calls = []
    inner = Fn._contrastive_items_kernel
    monkeypatch.setattr(Fn, "_contrastive_items_kernel", lambda src, lists: (calls.append((src.device.type, lists.n)), inner(src, lists))[1])
    return calls


def test_plugin_on_the_kernel_against_the_reference(g20, monkeypatch):
    calls = count_kernel_calls(monkeypatch)
    plugin, indices, got = g20.run(DEV)
    assert calls == [("cuda", len(g20.items()))]                # one call for the whole batch, on the kernel
    for f, per_video in enumerate(g20.matched()):
        for v, want in enumerate(per_video):
            assert torch.equal(torch.stack(indices[f][v]), want), (f, v)
    assert K.plain_items(plugin.last_items) == g20.items()
    ref32 = {"loss_reid": g20.t("f32/loss_reid"), "loss_aux_reid": g20.t("f32/loss_aux_reid"), "grad": g20.t("f32/grad_pred_reid_embed")}
    ref64 = {"loss_reid": g20.t("f64/loss_reid"), "loss_aux_reid": g20.t("f64/loss_aux_reid"), "grad": g20.t("f64/grad_pred_reid_embed")}
    K.check_4x(got, ref32, ref64, "g20 GPU ")
    _, _, again = g20.run(DEV)
    assert all(torch.equal(got[k], again[k]) for k in got)      # the same bits on every call


def test_plugin_on_the_torch_formulation(g20, monkeypatch):
    monkeypatch.setenv("DVIS_CONTRASTIVE_ITEMS", "0")
    calls = count_kernel_calls(monkeypatch)
    _, _, got = g20.run(DEV)
    assert not calls
    ref32 = {"loss_reid": g20.t("f32/loss_reid"), "loss_aux_reid": g20.t("f32/loss_aux_reid"), "grad": g20.t("f32/grad_pred_reid_embed")}
    ref64 = {"loss_reid": g20.t("f64/loss_reid"), "loss_aux_reid": g20.t("f64/loss_aux_reid"), "grad": g20.t("f64/grad_pred_reid_embed")}
    K.check_4x(got, ref32, ref64, "g20 GPU, torch formulation ")


def test_no_items_on_the_gpu(g20, monkeypatch):
    from dvis_plus_amd.matcher import HungarianMatcher
    calls = count_kernel_calls(monkeypatch)
    T = g20.meta["T"]
    det, plugin = g20.det_outputs(DEV), g20.plugin(replay=False)
    once = g20.targets(DEV)
    for e, t in enumerate(once):
        if e % T:
            t["ids"] = torch.full_like(t["ids"], -1)
    losses = plugin.train_loss(det, once, HungarianMatcher(num_points=g20.meta["points"], **g20.meta["weights"]))
    assert not calls and plugin.last_items == []
    for k in ("loss_reid", "loss_aux_reid"):
        assert float(losses[k].detach()) == 0.0 and losses[k].requires_grad and losses[k].is_cuda
    (g,) = torch.autograd.grad(losses["loss_reid"] + losses["loss_aux_reid"], det["pred_reid_embed"])
    assert torch.equal(g, torch.zeros_like(g))


def test_raises_on_the_gpu(g20):
    plugin = g20.plugin(num_negatives=g20.meta["Q"])
    with pytest.raises(ValueError, match="NUM_NEGATIVES"):
        plugin.train_loss(g20.det_outputs(DEV), g20.targets(DEV), g20.matcher())
    with pytest.raises(NotImplementedError, match="NOISE_EMBED"):
        g20.plugin(noise_embed=True)


def test_ctminvis_training_step(monkeypatch):
    calls = count_kernel_calls(monkeypatch)
    m = K.ctminvis_model(DEV)
    batch = minvis_batch(DEV)
    m.train()
    torch.manual_seed(3)
    losses = m(batch)
    assert calls == [("cuda", 2)]
    want = set(m.criterion.weight_dict) | {"loss_reid", "loss_aux_reid"}
    assert set(losses) == want and all(torch.isfinite(v).all() for v in losses.values())
    sum(losses.values()).backward()
    for n, p in m.sem_seg_head.predictor.reid_embed.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
    for n, p in m.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad).all(), n


def test_eval_aligns_on_the_reid_embeddings(g20):
    out, logits = eval_on_g20_clip(g20, DEV)
    check_eval_on_g20_clip(g20, out, logits)


def test_registry_resolves():
    from dvis_plus_amd import d2
    from dvis_plus_amd.registry import META_ARCH_REGISTRY
    d2._populate()
    assert META_ARCH_REGISTRY.get("CTMinVIS").__name__ == "CTMinVIS"
