"""CTVIS's segmenter stage on the CPU against g20 (the reference's own CTCLPlugin.train_loss and CTMinVIS.post_processing with the
recorded draws replayed through `_draw` / `_rand`): matched indices and the item table as integers, both losses and the gradient
to pred_reid_embed, the cases that raise, and CTMinVIS end to end at toy sizes."""
import numpy as np
import pytest
import torch

import ctvis_cases as K
from segmenter_train_cases import minvis_batch, minvis_model


@pytest.fixture(scope="module")
def g20():
    return K.G20()


def test_matched_indices_and_item_table_equal_the_reference(g20):
    plugin, indices, _ = g20.run()
    for f, per_video in enumerate(g20.matched()):
        for v, want in enumerate(per_video):
            assert torch.equal(torch.stack(indices[f][v]), want), (f, v)
    assert K.plain_items(plugin.last_items) == g20.items()
    kinds = [it["pos_sg"] for it in plugin.last_items]
    assert True in kinds and False in kinds
    # the fixture's planted cases: all-Q negatives behind an absent frame, a positive taken from after, a skipped item
    Q = g20.meta["Q"]
    assert any(len(it["neg"]) == Q for it in plugin.last_items) and any(len(it["neg"]) == Q - 1 for it in plugin.last_items)
    assert any(not it["pos_sg"] and it["pos"] > it["anchor"] for it in plugin.last_items)
    assert not any(it["video"] == 1 and it["instance"] == 1 for it in plugin.last_items)


def test_losses_and_gradient_equal_the_reference(g20):
    ref32 = {"loss_reid": g20.t("f32/loss_reid"), "loss_aux_reid": g20.t("f32/loss_aux_reid"), "grad": g20.t("f32/grad_pred_reid_embed")}
    ref64 = {"loss_reid": g20.t("f64/loss_reid"), "loss_aux_reid": g20.t("f64/loss_aux_reid"), "grad": g20.t("f64/grad_pred_reid_embed")}
    _, _, got64 = g20.run(dtype=torch.float64)
    for k in ref64:
        torch.testing.assert_close(got64[k], ref64[k], rtol=1e-10, atol=1e-12)
    _, _, got32 = g20.run()
    K.check_4x(got32, ref32, ref64, "g20 CPU fp32 ")
    # the similarity-guided rows carry gradient: without them the gradient differs
    assert float(ref64["grad"].abs().max()) > 0


def test_train_loss_weights_and_keys(g20):
    plugin, matcher = g20.plugin(), g20.matcher()
    det = g20.det_outputs()
    losses = plugin.train_loss(det, g20.targets(), matcher)
    assert set(losses) == {"loss_reid", "loss_aux_reid"}
    torch.testing.assert_close(losses["loss_reid"].detach(), g20.t("f32/loss_reid"), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(losses["loss_aux_reid"].detach(), g20.t("f32/loss_aux_reid"), rtol=1e-4, atol=1e-5)


def test_no_items_gives_zero_losses_with_a_graph(g20):
    T = g20.meta["T"]
    det, plugin = g20.det_outputs(), g20.plugin(replay=False)
    # (a) no instance at all
    empty = [{"labels": torch.zeros(0, dtype=torch.int64), "ids": torch.zeros(0, dtype=torch.int64),
              "masks": torch.zeros(0, g20.meta["H"], g20.meta["W"])} for _ in range(g20.meta["B"] * T)]
    # (b) nothing valid twice: every instance valid in frame 0 only
    once = g20.targets()
    for e, t in enumerate(once):
        if e % T:
            t["ids"] = torch.full_like(t["ids"], -1)
    for targets in (empty, once):
        from dvis_plus_amd.matcher import HungarianMatcher
        losses = plugin.train_loss(det, targets, HungarianMatcher(num_points=g20.meta["points"], **g20.meta["weights"]))
        assert plugin.last_items == []
        for k in ("loss_reid", "loss_aux_reid"):
            assert float(losses[k].detach()) == 0.0 and losses[k].requires_grad
        (g,) = torch.autograd.grad(losses["loss_reid"] + losses["loss_aux_reid"], det["pred_reid_embed"])
        assert torch.equal(g, torch.zeros_like(g))


def test_noise_embed_and_too_many_negatives_raise(g20):
    from dvis_plus_amd.criterion import CTCLPlugin, build_cl_plugin
    with pytest.raises(NotImplementedError, match="NOISE_EMBED"):
        g20.plugin(noise_embed=True)
    cfg = K.ctvis_cfg()
    cfg.MODEL.CL_PLUGIN.NOISE_EMBED = True
    with pytest.raises(NotImplementedError, match="NOISE_EMBED"):
        build_cl_plugin(cfg)
    plugin = g20.plugin(num_negatives=g20.meta["Q"])          # num_negatives + 1 > Q
    with pytest.raises(ValueError, match="NUM_NEGATIVES"):
        plugin.train_loss(g20.det_outputs(), g20.targets(), g20.matcher())
    cfg = K.ctvis_cfg()
    p = build_cl_plugin(cfg)
    assert isinstance(p, CTCLPlugin) and p.weight_dict == {"loss_reid": 2.0, "loss_aux_reid": 3.0}
    assert (p.num_negatives, p.sampling_frame_num, p.bio_cl, p.momentum_embed, p.noise_embed) == (99, 10, False, True, False)


def test_default_draws_follow_the_seeds(g20):
    """Without replay the draws are random.sample / np.random.rand: seeding both reproduces a run."""
    import random
    from dvis_plus_amd.criterion import CTCLPlugin
    p = CTCLPlugin(weight_dict={}, num_negatives=7, sampling_frame_num=4, bio_cl=False, momentum_embed=True, noise_embed=False)
    random.seed(5), np.random.seed(5)
    a = (p._draw("negatives", list(range(7)), 5), p._draw("momentum"))
    random.seed(5), np.random.seed(5)
    assert a == (random.sample(list(range(7)), 5), float(np.random.rand()))
    with pytest.raises(ValueError):
        p._draw("other")


# ---------------------------------------------------------------------------------------------------------- CTMinVIS
def test_registry_and_from_config():
    from dvis_plus_amd import config, d2
    from dvis_plus_amd.criterion import CTCLPlugin, VideoSetCriterion, build_criterion
    from dvis_plus_amd.matcher import HungarianMatcher, VideoHungarianMatcher
    from dvis_plus_amd.meta_architecture import CTMinVIS, MinVIS
    from dvis_plus_amd.registry import META_ARCH_REGISTRY
    d2._populate()
    assert META_ARCH_REGISTRY.get("CTMinVIS") is CTMinVIS and issubclass(CTMinVIS, MinVIS)
    cfg = K.ctvis_cfg()
    assert cfg.MODEL.META_ARCHITECTURE == "CTMinVIS"
    crit = build_criterion(cfg)
    assert isinstance(crit, VideoSetCriterion) and type(crit.matcher) is VideoHungarianMatcher
    assert crit.weight_dict == build_criterion(cfg, "MinVIS").weight_dict
    m = config.build_model(cfg)                                # the yaml's names through the registries
    assert type(m) is CTMinVIS and isinstance(m.cl_plugin, CTCLPlugin) and type(m.image_matcher) is HungarianMatcher
    mf = cfg.MODEL.MASK_FORMER
    assert (m.image_matcher.cost_class, m.image_matcher.cost_mask, m.image_matcher.cost_dice, m.image_matcher.num_points) == \
        (mf.CLASS_WEIGHT, mf.MASK_WEIGHT, mf.DICE_WEIGHT, mf.TRAIN_NUM_POINTS)
    assert m.cl_plugin.num_negatives == 99 and m.num_frames == 10
    assert type(m.sem_seg_head.predictor).__name__ == "VideoMultiScaleMaskedTransformerDecoder_dvisPlus"


def test_ctminvis_training_step():
    m = K.ctminvis_model()
    batch = minvis_batch()
    m.train()
    torch.manual_seed(3)
    losses = m(batch)
    want = set(m.criterion.weight_dict) | {"loss_reid", "loss_aux_reid"}
    assert set(losses) == want and all(torch.isfinite(v).all() for v in losses.values())
    assert len(m.cl_plugin.last_items) == 2                    # per video: the instance valid in both frames, at frame 1
    # the yaml's weights: the plugin's losses are its unweighted ones times 2 and 3
    sum(losses.values()).backward()
    for n, p in m.sem_seg_head.predictor.reid_embed.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
    plugin, m.cl_plugin = m.cl_plugin, None
    with pytest.raises(RuntimeError, match="cl_plugin"):
        m(batch)
    m.cl_plugin = plugin
    uneven = [dict(batch[0]), dict(batch[1], image=[f[:, :32] for f in batch[1]["image"]])]
    with pytest.raises(ValueError, match="one size"):
        m(uneven)


def test_plugin_losses_carry_the_configured_weights():
    m = K.ctminvis_model()
    batch = minvis_batch()
    m.train()

    def run(weights):
        m.cl_plugin.weight_dict = weights
        torch.manual_seed(3), np.random.seed(3)
        return m(batch)
    a, b = run({"loss_reid": 2.0, "loss_aux_reid": 3.0}), run({"loss_reid": 1.0, "loss_aux_reid": 1.0})
    torch.testing.assert_close(a["loss_reid"], 2.0 * b["loss_reid"])
    torch.testing.assert_close(a["loss_aux_reid"], 3.0 * b["loss_aux_reid"])
    assert torch.equal(a["loss_ce"], b["loss_ce"])


def eval_on_g20_clip(g20, device="cpu"):
    """The toy model's .eval() with the decoder heads replaced by the fixture's clip: logits and reid embeddings are the recorded
    ones, the decoder embeddings (masks only) random."""
    m = K.ctminvis_model(device)
    pp = g20.meta["pp"]
    logits, reid = g20.t("pp/in_logits")[0].to(device), g20.t("pp/in_reid")[0].permute(1, 2, 0).contiguous().to(device)    # (T,Q,K+1), (T,Q,C)
    pred = m.sem_seg_head.predictor
    m.sem_seg_head.num_classes = pp["K"]
    dec = torch.randn(pp["T"], pp["Q"], pred.decoder_norm.weight.shape[0], generator=torch.Generator().manual_seed(1)).to(device)
    pred._final_heads = lambda output, mask_features, need_masks: (dec, logits, None)

    class RecordedReid(torch.nn.Module):
        def forward(self, d):
            assert d is dec
            return reid
    pred.reid_embed = RecordedReid()
    g = torch.Generator().manual_seed(2)
    frames = [(torch.rand(3, 64, 96, generator=g) * 255).to(device) for _ in range(pp["T"])]
    return m([{"image": frames, "height": 64, "width": 96}]), logits


def check_eval_on_g20_clip(g20, out, logits):
    perms = g20.z["pp/perms"]                                  # (T - 1, Q): frame t's permutation
    idx = out["aligned_indices"].cpu()
    assert idx[0].tolist() == list(range(idx.shape[1]))
    assert np.array_equal(idx[1:].numpy(), perms)              # bit-exact
    T = idx.shape[0]
    aligned = logits.cpu()[torch.arange(T)[:, None], idx].mean(0)
    torch.testing.assert_close(aligned, g20.t("pp/logits")[0], rtol=0, atol=1e-3)
    scores = torch.softmax(g20.t("pp/logits")[0], -1)[:, :-1].flatten().topk(10)[0]
    torch.testing.assert_close(torch.tensor(sorted(out["pred_scores"], reverse=True)), scores, rtol=0, atol=1e-3)


def test_eval_aligns_on_the_reid_embeddings(g20):
    out, logits = eval_on_g20_clip(g20)
    check_eval_on_g20_clip(g20, out, logits)


def test_minvis_eval_is_unchanged_by_the_hook():
    from tracker_train_cases import same_output
    from dvis_plus_amd.tracker import match_chain
    m, _ = minvis_model(criterion=False)
    video = [{k: v for k, v in minvis_batch()[0].items() if k != "instances"}]
    before = m(video)
    from dvis_plus_amd.meta_architecture import CTMinVIS        # noqa: F401
    seen = []
    pred = m.sem_seg_head.predictor
    inner = pred._final_heads
    pred._final_heads = lambda *a: (seen.append(inner(*a)), seen[-1])[1]
    after = m(video)
    assert same_output(after, before)
    dec = seen[-1][0]
    nrm = dec / dec.norm(dim=-1, keepdim=True)                 # the chain as it stood before the hook, on the decoder embeddings
    chain = match_chain(1 - torch.bmm(nrm[1:], nrm[:-1].transpose(1, 2)))
    assert np.array_equal(after["aligned_indices"][1:].numpy(), chain)
