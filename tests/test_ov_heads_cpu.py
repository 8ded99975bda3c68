"""The open-vocabulary (FC-CLIP) classification path on CPU tensors: the cpu_ops formulations of mask_pool / text_class_logits /
ov_ensemble and the `_OV` decoders against golden g22 (the reference's own modules), the state-dict layout, construction through
the registries, and the refusals.  No GPU."""
import json
import os

import pytest
import torch

import ov_heads_cases as C
from dvis_plus_amd import cpu_ops, d2, functions as Fn
from dvis_plus_amd import transformer_decoder as td
from dvis_plus_amd.registry import SEM_SEG_HEADS_REGISTRY, TRANSFORMER_DECODER_REGISTRY, ShapeSpec

TOL = dict(rtol=1e-5, atol=1e-5)


def test_mask_pool_and_module_reproduce_the_reference():
    g = C.g22()
    x, mask = g.t("direct/x"), g.t("direct/mask")
    total, count = Fn.mask_pool(x, mask)
    assert count.dtype == torch.int32 and torch.equal(count, (mask > 0).sum((-1, -2)).to(torch.int32))
    pooled, denorm = Fn.mask_pool_mean(x, mask)
    torch.testing.assert_close(pooled, g.t("direct/pooled"), **TOL)
    torch.testing.assert_close(denorm, g.t("direct/denorm"), rtol=0, atol=0)
    torch.testing.assert_close(total / denorm.flatten(2), pooled, rtol=0, atol=0)
    mp = td.MaskPooling()
    torch.testing.assert_close(mp(x, mask), g.t("direct/pooled"), **TOL)
    got, num = mp(x=x, mask=mask, return_num=True)
    assert torch.equal(got, pooled) and torch.equal(num, denorm)
    # a mask of another size is resized with torch first, as in the reference
    small = mask[..., ::2, ::2].contiguous()
    want = Fn.mask_pool_mean(x, torch.nn.functional.interpolate(small, size=x.shape[-2:], mode="bilinear", align_corners=False))[0]
    assert torch.equal(mp(x, small), want)


def test_mask_pool_threshold_and_dtypes():
    x = torch.arange(2 * 4 * 2 * 3, dtype=torch.float64).view(2, 4, 2, 3)
    logits = torch.tensor([0.0, -0.0, 5e-324, float("nan"), 1.0, -1.0], dtype=torch.float64).view(1, 1, 2, 3).repeat(2, 2, 1, 1)
    total, count = Fn.mask_pool(x, logits)
    assert total.dtype == torch.float64 and count.tolist() == [[2, 2], [2, 2]]                 # the denormal and 1.0
    assert torch.equal(total[0, 0], x[0, :, 0, 2] + x[0, :, 1, 1])
    empty = Fn.mask_pool_mean(x.float(), -torch.ones(2, 3, 2, 3))
    assert torch.equal(empty[0], torch.zeros(2, 3, 4)) and torch.equal(empty[1], torch.full((2, 3, 1, 1), 1e-8))
    t, c = Fn.mask_pool(x.bfloat16(), logits.bfloat16())
    assert t.dtype == torch.bfloat16 and c.dtype == torch.int32


def test_text_class_logits_reproduce_the_reference():
    g = C.g22()
    got = Fn.text_class_logits(g.t("direct/emb"), g.t("in/text"), g.t("direct/logit_scale"), g.templates)
    torch.testing.assert_close(got, g.t("direct/logits"), **TOL)
    assert torch.equal(td.get_classification_logits(g.t("direct/emb"), g.t("in/text"), g.t("direct/logit_scale"), g.templates), got)
    out_vocab = Fn.text_class_logits(g.t("direct/clip_pooled"), g.t("in/text"), g.t("direct/clip_logit_scale"), g.templates)
    torch.testing.assert_close(out_vocab, g.t("ens/out_logits"), **TOL)
    # the clamp: exp(5) > 100
    hot = Fn.text_class_logits(g.t("direct/emb"), g.t("in/text"), torch.tensor(5.0), g.templates)
    unit = Fn.text_class_logits(g.t("direct/emb"), g.t("in/text"), torch.tensor(0.0), g.templates)
    torch.testing.assert_close(hot, 100 * unit, rtol=1e-6, atol=1e-5)
    assert Fn.text_class_logits(g.t("direct/emb").double(), g.t("in/text").double(), torch.tensor(2.1), g.templates).dtype == torch.float64


@pytest.mark.parametrize("valid", [False, True])
def test_ov_ensemble_reproduces_the_reference(valid):
    g = C.g22()
    v = g.t("direct/valid") if valid else None
    got = Fn.ov_ensemble(g.t("eval/pred_logits")[0], g.t("ens/out_logits"), g.t("direct/overlapping"), g.meta["alpha"], g.meta["beta"], v)
    torch.testing.assert_close(got, g.t("ens/valid" if valid else "ens/plain"), **TOL)
    # the log-domain form is the reference's formula: in float64 they agree to rounding
    a, b = g.t("eval/pred_logits")[0].double(), g.t("ens/out_logits").double()
    torch.testing.assert_close(cpu_ops.ov_ensemble(a, b, g.t("direct/overlapping"), 0.4, 0.8, v),
                               C.reference_ensemble(a, b, g.t("direct/overlapping"), 0.4, 0.8, v), rtol=1e-12, atol=1e-12)


def test_ov_ensemble_is_finite_at_clip_scale_where_the_reference_is_not():
    gen = torch.Generator().manual_seed(5)
    a, b = 100 * (2 * torch.rand(9, 41, generator=gen) - 1), 100 * (2 * torch.rand(9, 41, generator=gen) - 1)
    ov = (torch.rand(40, generator=gen) < 0.5).float()
    got = Fn.ov_ensemble(a, b, ov, 0.4, 0.8)
    assert torch.isfinite(got).all() and (got >= torch.log(torch.tensor(1e-8))).all()
    torch.testing.assert_close(got.double(), C.reference_ensemble(a.double(), b.double(), ov, 0.4, 0.8), rtol=1e-4, atol=1e-4)
    p = a[..., :-1].softmax(-1)                                                  # the reference in fp32: log 0 times the other mask
    assert not torch.isfinite(((p ** 0.6 * b[..., :-1].softmax(-1) ** 0.4).log() * ov)).all()
    # alpha = beta = 0: the in-vocabulary distribution with void re-attached
    p_void = a.softmax(-1)[..., -1:]
    want = torch.log(torch.cat([a[..., :-1].softmax(-1) * (1 - p_void), p_void], -1) + 1e-8)
    torch.testing.assert_close(Fn.ov_ensemble(a, b, ov, 0.0, 0.0), want, rtol=1e-5, atol=1e-5)


def test_state_dict_keys_and_shapes_equal_the_reference():
    g = C.g22()
    with open(os.path.join(C.GOLDEN, "ref_state_shapes_ov_decoder.json")) as f:
        want = json.load(f)
    for cls in (C.DVIS_OV, C.MINVIS_OV):
        dec = C.build_decoder(g, cls=cls)                                        # strict load inside
        assert {k: list(v.shape) for k, v in dec.state_dict().items()} == want
    assert "logit_scale" in want and "class_embed.layers.2.weight" in want and "_mask_pooling_proj.1.weight" in want
    assert "class_embed.weight" not in want


def test_decoder_train_mode_under_no_grad_reproduces_every_prediction():
    g = C.g22()
    out, pooled = C.run_decoder(g, C.build_decoder(g), train=True)
    assert out["pred_logits"].shape == (2, 2, 6, 6) and out["pred_masks"].shape == (2, 6, 2, 8, 16)
    assert len(out["aux_outputs"]) == g.meta["layers"]
    C.check_train_outputs(g, out, pooled, TOL)


def test_decoder_eval_reproduces_the_reference_and_is_the_last_training_prediction():
    g = C.g22()
    dec = C.build_decoder(g)
    out, pooled = C.run_decoder(g, dec, train=False)
    assert out["pred_logits"].shape == (1, 4, 6, 6) and out["pred_masks"].shape == (1, 6, 4, 8, 16) and len(pooled) == 1
    assert out["pred_embds"].shape == (1, 64, 4, 6) and out["mask_features"].shape == (4, 64, 8, 16)
    C.check_eval_outputs(g, out, TOL)
    tr, tr_pooled = C.run_decoder(g, dec, train=True)
    assert torch.equal(out["pred_logits"][0], tr["pred_logits"].flatten(0, 1))
    assert torch.equal(out["pred_masks"][0].transpose(0, 1), tr["pred_masks"].transpose(1, 2).flatten(0, 1))
    assert torch.equal(pooled[0][0], tr_pooled[-1][0]) and torch.equal(pooled[0][1], tr_pooled[-1][1])


def test_minvis_ov_drops_mask_features():
    g = C.g22()
    out, _ = C.run_decoder(g, C.build_decoder(g, cls=C.MINVIS_OV), train=False)
    assert "mask_features" not in out
    C.check_eval_outputs(g, out, TOL)


def test_built_through_the_registries_from_a_cfg_with_fc_clip():
    from dvis_plus_amd.config import get_default_cfg
    fc = get_default_cfg().MODEL.FC_CLIP                                          # ov_dvis/config.py:16-22
    assert (fc.CLIP_MODEL_NAME, fc.CLIP_PRETRAINED_WEIGHTS, fc.EMBED_DIM) == ("convnext_large_d_320", "laion2b_s29b_b131k_ft_soup", 768)
    assert (fc.GEOMETRIC_ENSEMBLE_ALPHA, fc.GEOMETRIC_ENSEMBLE_BETA, fc.ENSEMBLE_ON_VALID_MASK) == (0.4, 0.8, False)
    for name in (C.DVIS_OV, C.MINVIS_OV):
        cfg = C.ov_cfg(name)
        dec = d2.build_transformer_decoder(cfg, 64, True)
        assert type(dec).__name__ == name and TRANSFORMER_DECODER_REGISTRY.get(name) is type(dec)
        assert dec.class_embed.layers[-1].out_features == 24 and dec.num_layers == 4 and dec.num_frames == 2
        assert float(dec.logit_scale.detach()) == pytest.approx(2.6592600, abs=1e-6)      # log(1 / 0.07)
    shape = {f"res{i}": ShapeSpec(channels=8 * 2 ** i, stride=2 ** i) for i in (2, 3, 4, 5)}
    head = d2.build_sem_seg_head(C.ov_cfg(), shape)
    assert type(head) is SEM_SEG_HEADS_REGISTRY.get("FCCLIPHead") and type(head.predictor).__name__ == C.DVIS_OV
    assert head.num_classes == 5 and head.transformer_in_feature == "multi_scale_pixel_decoder"

    class Decoder(torch.nn.Module):                                              # the head passes the text classifier through
        def forward_features(self, features):
            return "mask_features", None, ["a", "b", "c"]

    class Predictor(torch.nn.Module):
        def forward(self, *a, **k):
            seen.update(args=a, **k)
            return "predictions"
    seen = {}
    head.pixel_decoder, head.predictor = Decoder(), Predictor()
    assert head({"res2": 0, "text_classifier": "T", "num_templates": [1, 1]}) == "predictions"
    assert seen == {"args": (["a", "b", "c"], "mask_features", None), "text_classifier": "T", "num_templates": [1, 1]}


def test_install_registers_the_ov_classes():
    """d2.install() copies every entry of the package's registries into detectron2's / the reference's: the new classes are entries."""
    d2._populate()
    assert {C.DVIS_OV, C.MINVIS_OV} <= {k for k, _ in TRANSFORMER_DECODER_REGISTRY.items()}
    assert "FCCLIPHead" in {k for k, _ in SEM_SEG_HEADS_REGISTRY.items()}


def test_refusals():
    g = C.g22()
    emb, text = g.t("direct/emb"), g.t("in/text")
    with pytest.raises(RuntimeError, match="num_templates.*add.*up to the 10 rows"):
        Fn.text_class_logits(emb, text, torch.tensor(1.0), [2, 1, 3, 1, 2, 2])
    with pytest.raises(RuntimeError, match="num_templates"):
        Fn.text_class_logits(emb, text, torch.tensor(1.0), [2, 1, 3, 0, 3, 1])    # an empty group
    # the served shapes of the kernel, asked of the library
    assert Fn.mask_pool_plan(1, 256, 2048, 184, 320) == Fn.MaskPoolPlan(slab=512, slabs=115)
    assert Fn.mask_pool_plan(5, 100, 4, 1, 1).slabs == 1
    with pytest.raises(RuntimeError, match="Q=257"):
        Fn.mask_pool_plan(1, 257, 256, 8, 16)
    with pytest.raises(RuntimeError, match="C=6"):
        Fn.mask_pool_plan(1, 6, 6, 8, 16)
    with pytest.raises(RuntimeError, match="C=2052"):
        Fn.mask_pool_plan(1, 6, 2052, 8, 16)
    with pytest.raises(RuntimeError, match="2\\^31 bytes"):
        Fn.mask_pool_plan(1, 6, 2048, 1024, 1024)
    with pytest.raises(RuntimeError, match="one map size"):
        Fn.mask_pool(torch.zeros(1, 4, 5, 7), torch.zeros(1, 3, 5, 8))
    # grad enabled with a trainable parameter: the heads have no backward
    dec = C.build_decoder(g)
    x, mf, text = g.inputs()
    for mode in (True, False):
        dec.train(mode)
        with pytest.raises(NotImplementedError, match="mask_pool and text_class_logits have no.*backward"):
            dec(x, mf, None, text_classifier=text, num_templates=g.templates)
    with pytest.raises(ValueError, match="text_classifier"):
        with torch.no_grad():
            dec(x, mf)
    for p in dec.parameters():                                                   # frozen: nothing to train, the forward runs
        p.requires_grad_(False)
    C.check_eval_outputs(g, dec.eval()(x, mf, None, text_classifier=text, num_templates=g.templates), TOL)
