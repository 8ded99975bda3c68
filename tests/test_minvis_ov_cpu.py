"""MinVIS_OV's host logic on CPU tensors against golden g23 — the reference's own MinVIS_OV forward on its own CLIP backbone
(tests/golden/gen_minvis_ov_golden.py) — with the HIP ops' CPU stand-ins (`oracle_ops`), and the class-name handling."""
import pytest
import torch

import minvis_ov_cases as M
from dvis_plus_amd import config, d2
from dvis_plus_amd import meta_architecture as MA

TOL = dict(rtol=1e-4, atol=1e-4)


def test_state_dict_is_the_references():
    model, g, meta = M.build(False)
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == M.state_shapes()
    assert {"void_embedding.weight", "additional_void_embedding.weight"} <= set(got)
    assert any(k.startswith("backbone.clip_model.") for k in got) and any(k.startswith("sem_seg_head.") for k in got)
    assert not any(p.requires_grad for p in model.backbone.parameters())
    assert MA.META_ARCH_REGISTRY.get("MinVIS_OV") is MA.MinVIS_OV and len(MA.VILD_PROMPT) == 14


@pytest.mark.parametrize("flag", [False, True], ids=["plain", "ENSEMBLE_ON_VALID_MASK"])
def test_forward_against_the_references(oracle_ops, flag):
    model, g, meta = M.build(flag)
    out, stages = M.run(model, g, meta)
    want = M.check_against_golden(stages, g, "valid" if flag else "plain", TOL)
    assert torch.equal(model.category_overlapping_mask, want["category_overlapping_mask"])
    assert len(out["pred_scores"]) == 10 and len(out["pred_masks"]) == 10 and tuple(out["image_size"]) == tuple(meta["out_hw"])
    assert out["pred_masks"][0].shape == (meta["T"], *meta["out_hw"])


def test_class_names_templates_and_overlap():
    model, g, meta = M.build(False)
    prep = model.test_class_prepares[M.NAME]
    assert prep["num_templates"] == [2, 1, 3, 1, 2] and prep["overlapping"].tolist() == [1, 0, 1, 0, 0]
    assert len(prep["class_names"]) == 9 * 14 and prep["class_names"][0] == "a photo of a dog." \
        and prep["class_names"][14] == "a photo of a hound."
    assert model.train_names2id == {"toy_train_a": 0, "toy_train_b": 1}
    model.set_metadata("other", M.metadata(["road", "zebra"]))
    assert model.test_class_prepares["other"]["overlapping"].tolist() == [1, 0]


def test_void_rows_by_dataset_and_merge_mode():
    model, g, meta = M.build(False)
    text = torch.nn.functional.normalize(torch.randn(9, 24), dim=-1)
    nt = [2, 1, 3, 1, 2]
    norm = lambda w: torch.nn.functional.normalize(w, dim=-1)
    with torch.no_grad():
        void0, void1 = norm(model.void_embedding.weight), norm(model.additional_void_embedding.weight)
        for name, want in (("toy_train_a", void0), ("toy_train_b", void1), (M.NAME, void0)):      # 'coco': the first void embedding
            tc, n = model.get_text_classifier_with_void(text, nt, name)
            assert n == nt + [1] and torch.equal(tc[:9], text) and torch.equal(tc[9:], want), name
        model.void_embedding_merge_mode = "mean"
        tc, n = model.get_text_classifier_with_void(text, nt, M.NAME)
        assert n == nt + [1] and torch.allclose(tc[9:], torch.cat([void0, void1]).mean(0, keepdim=True))
        model.void_embedding_merge_mode = "max"
        tc, n = model.get_text_classifier_with_void(text, nt, M.NAME)
        assert n == nt + [2] and torch.equal(tc[9:], torch.cat([void0, void1]))
        # all vocabulary: the training synonyms that share no name with the test classes join the void group
        model.void_embedding_merge_mode = "coco"
        model.test_use_all_vocabulary = True
        own, own_n = model._set_class_information(M.NAME, False)
        tc, n = model.get_text_classifier_with_void(own, own_n, M.NAME)
        # training synonyms: cat | dog, puppy | tree | car, automobile | road; "dog, puppy" and "tree" overlap -> 4 rows join
        assert n == nt + [1 + 4] and tc.shape[0] == 9 + 1 + 4


def test_set_text_classifier_needs_no_tokenizer(oracle_ops):
    model, g, meta = M.build(False, tokenizer=False)
    with pytest.raises(RuntimeError, match="CLIP.text_tokenizer is not set"):
        model([M.video(g, meta)])
    want = torch.from_numpy(g.z["plain/text_classifier"].copy())
    model.set_text_classifier(M.NAME, want[:9], [2, 1, 3, 1, 2], [1, 0, 1, 0, 0])
    out, stages = M.run(model, g, meta)
    M.check_against_golden(stages, g, "plain", TOL)
    with pytest.raises(ValueError, match="set_text_classifier"):
        model.set_text_classifier(M.NAME, want[:8], [2, 1, 3, 1, 2], [1, 0, 1, 0, 0])


def test_training_raises_and_no_grad_train_mode_is_eval(oracle_ops):
    model, g, meta = M.build(False)
    ref, _ = M.run(model, g, meta)
    model.train()
    with pytest.raises(NotImplementedError, match="MinVIS_OV does not train"):
        model([M.video(g, meta)])
    model.eval()
    again, _ = M.run(model, g, meta)
    assert again["pred_scores"] == ref["pred_scores"] and again["pred_labels"] == ref["pred_labels"]


def test_build_model_from_an_open_vocabulary_config():
    """A configs/open_vocabulary/FC-CLIP_*_convnextl.yaml-shaped config through d2.build_model, on the meta device (no weights)."""
    cfg = config.get_default_cfg()
    cfg.merge(dict(MODEL=dict(META_ARCHITECTURE="MinVIS_OV", BACKBONE=dict(NAME="CLIP"),
                              SEM_SEG_HEAD=dict(NAME="FCCLIPHead", NUM_CLASSES=133),
                              MASK_FORMER=dict(TRANSFORMER_DECODER_NAME="VideoMultiScaleMaskedTransformerDecoder_minvis_OV",
                                               SIZE_DIVISIBILITY=32, TEST=dict(TASK="vps", WINDOW_INFERENCE=True))),
                   DATASETS=dict(TRAIN=["toy_train_a"], TEST=[M.NAME], TEST2TRAIN=["toy_train_a"])))
    for name, names in (("toy_train_a", ["cat", "dog, puppy"]), (M.NAME, ["dog", "sky"])):
        MA.OV_METADATA[name] = M.metadata(names)
    try:
        with torch.device("meta"):
            model = d2.build_model(cfg)
    finally:
        MA.OV_METADATA.clear()
    assert isinstance(model, MA.MinVIS_OV) and model.task == "vps" and model.additional_void_embedding is None
    assert model.backbone.model_name == "convnext_large_d_320" and model.void_embedding.weight.shape == (1, 768)
    assert model.test2train == {M.NAME: "toy_train_a"} and model.test_class_prepares[M.NAME]["num_templates"] == [1, 1]
    MA.OV_METADATA.clear()
    with pytest.raises(KeyError, match="OV_METADATA"):
        with torch.device("meta"):
            d2.build_model(cfg)
