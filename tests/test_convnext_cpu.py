"""The CLIP ConvNeXt backbone's host side on CPU tensors (dvis_plus_amd/convnext.py): state-dict names and shapes against the
committed fixture, the reference's backbone surface, and a toy trunk / head / text tower against the LITERAL timm / open_clip
composition of convnext_cases.py (grouped conv2d on NCHW, permute, layer_norm, linear, gelu, gamma * ..., nn.MultiheadAttention under
the causal mask) within rtol = atol = 1e-5, as the Swin fixtures are compared on the CPU."""
import ctypes
import json
import os

import pytest
import torch

import convnext_cases as K
from dvis_plus_amd import config, d2, functions as Fn, native
from dvis_plus_amd.convnext import CLIP
from dvis_plus_amd.registry import BACKBONE_REGISTRY
from segmenter_train_cases import MIN_SAMPLES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = dict(rtol=1e-5, atol=1e-5)
OUTS = ("stem", "res2", "res3", "res4", "res5")


def clip_cfg(name="convnext_large_d_320"):
    cfg = config.get_default_cfg()
    cfg.MODEL.BACKBONE.NAME = "CLIP"
    cfg.MODEL.FC_CLIP.CLIP_MODEL_NAME = name
    return cfg


def toy_pair(head, seed=0):
    """(this package's CLIP, the literal CLIP) at the toy sizes with ONE seeded state dict, every parameter off its initial value."""
    lit = K.randomize_(K.LitCLIP(**K.toy_model_cfg(head)), seed).eval()
    ours = CLIP(clip_cfg(), model_cfg=K.toy_model_cfg(head))
    ours.clip_model.load_state_dict(lit.state_dict(), strict=True)
    return ours, lit


@pytest.mark.parametrize("name", ["convnext_base_w", "convnext_large_d_320"])
def test_state_dict_names_and_shapes(name):
    with open(os.path.join(GOLDEN, "ref_state_shapes_clip_convnext.json")) as f:
        want = json.load(f)[name]
    with torch.device("meta"):
        model = d2.build_backbone(clip_cfg(name))
    assert isinstance(model, CLIP) and BACKBONE_REGISTRY.get("CLIP") is CLIP
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == want, (sorted(set(got) ^ set(want))[:10], [k for k in got if k in want and got[k] != want[k]][:10])
    assert not any(p.requires_grad for p in model.parameters()) and not model.training
    assert "clip_model.attn_mask" not in got and model.clip_model.attn_mask.shape == (77, 77)      # a non-persistent buffer


@pytest.mark.parametrize("name,dims,embed", [("convnext_base_w_320", (128, 256, 512, 1024), 640), ("convnext_large_d", (192, 384, 768, 1536), 768)])
def test_backbone_surface(name, dims, embed):
    with torch.device("meta"):
        m = CLIP(clip_cfg(name), None)
    assert m.model_name == name and m.dim_latent == embed and m.size_divisibility == -1 and m.text_tokenizer is None
    shape = m.output_shape()
    assert list(shape) == ["stem", "res2", "res3", "res4", "res5", "clip_embedding"]
    assert [shape[k].channels for k in shape] == [dims[0], *dims, embed]
    assert [shape[k].stride for k in shape] == [2, 4, 8, 16, 32, -1]


@pytest.mark.parametrize("name", ["RN50", "RN50x4", "convnext_xxlarge"])
def test_models_that_are_not_built_raise_naming_the_key(name):
    with pytest.raises(NotImplementedError, match="MODEL.FC_CLIP.CLIP_MODEL_NAME") as e:
        CLIP(clip_cfg(name), None)
    assert name in str(e.value)


@pytest.mark.parametrize("head", ["linear", "mlp"])
@pytest.mark.parametrize("pad_to", [64, None], ids=["padded to 64", "37 x 53 as it is"])
def test_toy_trunk_and_head_match_the_literal_composition(head, pad_to):
    ours, lit = toy_pair(head)
    x = K.toy_frames(pad_to=pad_to)
    with torch.no_grad():
        want = lit.extract_features(x)
    got = ours(x)
    assert set(got) == {*OUTS, "clip_vis_dense"}
    for k in (*OUTS, "clip_vis_dense"):
        assert got[k].shape == want[k].shape and got[k].is_contiguous(), k
        torch.testing.assert_close(got[k], want[k], **TOL, msg=lambda m: f"{k}: {m}")
    pooled = torch.randn(2, 6, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        torch.testing.assert_close(ours.visual_prediction_forward(pooled), lit.visual_prediction_forward(pooled), **TOL)
    assert ours.visual_prediction_forward(pooled).shape == (2, 6, 24)


def test_encode_text_matches_the_literal_tower():
    ours, lit = toy_pair("linear", seed=1)
    tokens = K.toy_tokens()
    assert len(set(tokens.argmax(-1).tolist())) == tokens.shape[0]
    with torch.no_grad():
        want = lit.encode_text(tokens)
        got = ours.encode_text(tokens)
        torch.testing.assert_close(got, want, **TOL)
        torch.testing.assert_close(ours.encode_text(tokens, normalize=True), torch.nn.functional.normalize(want, dim=-1), **TOL)
    ours.text_tokenizer = lambda texts: tokens[:len(texts)]
    torch.testing.assert_close(ours.get_text_classifier(["a", "b", "c"], "cpu"), want[:3], **TOL)


def test_tokenize_text_without_a_tokenizer_says_what_to_do():
    ours, _ = toy_pair("linear")
    with pytest.raises(RuntimeError, match="CLIP.text_tokenizer is not set") as e:
        ours.tokenize_text(["a photo of a cat"])
    assert "open_clip.get_tokenizer" in str(e.value)
    with pytest.raises(RuntimeError, match="CLIP.text_tokenizer is not set"):
        ours.get_text_classifier(["a photo of a cat"], "cpu")


def test_gamma_fold_follows_an_in_place_weight_update():
    ours, lit = toy_pair("mlp", seed=2)
    x = K.toy_frames(seed=4)
    ours(x)                                                                                   # the folds exist now
    blk = ours.clip_model.visual.trunk.stages[2].blocks[1]
    before = blk.fc2_scaled()[0]
    with torch.no_grad():
        for m in (ours.clip_model, lit):
            m.visual.trunk.stages[2].blocks[1].gamma.mul_(-1.7)
            m.visual.trunk.stages[0].blocks[0].mlp.fc2.weight.add_(0.05)
        want = lit.extract_features(x)
    got = ours(x)
    for k in OUTS:
        torch.testing.assert_close(got[k], want[k], **TOL, msg=lambda m: f"{k}: {m}")
    assert blk.fc2_scaled()[0].data_ptr() == before.data_ptr()                                # refreshed in place: graphs keep their pointer


def test_trunk_is_frozen_and_inference_only():
    ours, _ = toy_pair("linear")
    x = K.toy_frames(seed=5)
    ref = ours(x)
    ours.train()
    with torch.no_grad():
        again = ours.extract_features(x)
    assert all(torch.equal(again[k], ref[k]) for k in OUTS)                                   # .train() under no_grad: the same bits
    ours.clip_model.visual.trunk.stages[1].blocks[0].gamma.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="does not train"):
        ours.extract_features(x)
    out = ours(x)                                                                             # forward is always eval + no_grad (clip.py:214-217)
    assert not ours.training and all(torch.equal(out[k], ref[k]) and not out[k].requires_grad for k in OUTS)


def test_dwconv_ln_op_on_cpu_tensors_is_the_literal_composition():
    d = K.cast(K.dwconv_ln_inputs(2, 5, 9, 12), torch.float32)
    conv = torch.nn.Conv2d(12, 12, 7, padding=3, groups=12)
    norm = torch.nn.LayerNorm(12, eps=K.EPS)
    with torch.no_grad():
        conv.weight.copy_(d["weight"]), conv.bias.copy_(d["bias"]), norm.weight.copy_(d["gamma"]), norm.bias.copy_(d["beta"])
        want = K.dwconv_ln_literal(**d)
        torch.testing.assert_close(Fn.dwconv7x7_ln_tokens(d["x"], conv, norm), want, **TOL)
        torch.testing.assert_close(Fn.dwconv7x7_ln_tokens(d["x"].view(2, 45, 12), conv, norm, hw=(5, 9)), want.view(2, 45, 12), **TOL)
    with pytest.raises(RuntimeError, match="expected x"):
        Fn.dwconv7x7_ln_tokens(d["x"].view(2, 45, 12), conv, norm, hw=(5, 8))


@pytest.mark.parametrize("shape", [s for s in K.DWCONV_LN_SHAPES.values() if s[0] * s[1] * s[2] * s[3] >= MIN_SAMPLES])
def test_variance_shortcut_would_fail(shape):
    """On the inputs of test_dwconv_ln_gpu.py the literal fp32 run stays finite, and E[z^2] - mean^2 in fp32 is more than 4 x as far
    from the fp64 run as the literal fp32 run is: a kernel taking that shortcut cannot pass the 4 x rule there."""
    d = K.dwconv_ln_inputs(*shape)
    ref64 = K.dwconv_ln_literal(**d)
    d32 = K.cast(d, torch.float32)
    lit32 = K.dwconv_ln_literal(**d32)
    assert torch.isfinite(lit32).all()
    base = (lit32.double() - ref64).abs().max().item()
    short = (K.dwconv_ln_shortcut(**d32).double() - ref64).abs().max().item()
    print(f"{shape}: fp32 literal {base:.3e}, fp32 shortcut {short:.3e}, ratio {short / base:.1f}")
    assert short > 4 * base


def test_dwconv_ln_refusals_through_the_c_abi():
    K.check_dwconv_ln_refusals(native.lib(), ctypes)
