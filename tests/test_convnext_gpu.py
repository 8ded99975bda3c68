"""The CLIP ConvNeXt backbone on the GPU (dvis_plus_amd/convnext.py on csrc/dwconv_ln.hip and the project's GEMM kernels) against
the LITERAL timm / open_clip composition of convnext_cases.py run on the CPU in fp64, at the project's 4 x rule per output (`check_4x`:
the GPU result may be 4 x as far from the fp64 run as the fp32 CPU run of the same literal composition is) — once with the split-f16
GEMM path on and once under ``Fn.x3_disabled()`` (the exact-fp32 path through the same modules)."""
import contextlib
import copy
import functools

import pytest
import torch

import convnext_cases as K
from dvis_plus_amd import config, functions as Fn
from dvis_plus_amd.convnext import CLIP
from vit_adapter_train_cases import check_4x

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUTS = ("stem", "res2", "res3", "res4", "res5")
# one block per stage at the widths of convnext_large_d: the smallest model that reaches the 1536-wide kernel, the > 1024
# LayerNorm branch (head.norm) and the tiled GEMMs (4 C hidden) together
WIDE = dict(dims=(192, 384, 768, 1536), depths=(1, 1, 1, 1), embed=768, head="mlp", text=(32, 2, 1), context=9, vocab=50)


def _cfg():
    cfg = config.get_default_cfg()
    cfg.MODEL.BACKBONE.NAME = "CLIP"
    return cfg


def _literal_outputs(lit, x, pooled):
    with torch.no_grad():
        out = {k: v for k, v in lit.extract_features(x).items() if k in OUTS}
        out["embedding"] = lit.visual_prediction_forward(pooled)
    return out


@functools.lru_cache(maxsize=None)
def case(kind, head):
    """(GPU model, GPU inputs, fp32 CPU literal outputs, fp64 CPU literal outputs), computed once per case and never modified."""
    mc = K.toy_model_cfg(head) if kind == "toy" else dict(WIDE, head=head)
    lit = K.randomize_(K.LitCLIP(**mc), seed=7).eval()
    if kind == "toy":
        x = K.toy_frames(seed=1)                                                                  # 2 x 3 x 37 x 53, padded to 64
    else:
        x = torch.randn(2, 3, 128, 160, generator=torch.Generator().manual_seed(2))               # maps 32 x 40 ... 4 x 5; stage 3: 8 x 10
    pooled = torch.randn(2, 6, mc["dims"][-1], generator=torch.Generator().manual_seed(3))
    cpu32 = _literal_outputs(lit, x, pooled)
    cpu64 = _literal_outputs(copy.deepcopy(lit).double(), x.double(), pooled.double())
    ours = CLIP(_cfg(), model_cfg=mc)
    ours.clip_model.load_state_dict(lit.state_dict(), strict=True)
    return ours.to(DEV), x.to(DEV), pooled.to(DEV), cpu32, cpu64


def _run(kind, head, exact):
    ours, x, pooled, cpu32, cpu64 = case(kind, head)
    with (Fn.x3_disabled() if exact else contextlib.nullcontext()):
        got = {k: v for k, v in ours(x).items() if k in OUTS}
        assert torch.equal(ours(x)["clip_vis_dense"], got["res5"])
        with torch.no_grad():
            got["embedding"] = ours.visual_prediction_forward(pooled)
    assert all(v.is_contiguous() and v.shape == cpu64[k].shape for k, v in got.items())
    check_4x(got, cpu32, cpu64, f"{kind} {head} {'exact' if exact else 'split-f16'} ")


@pytest.mark.parametrize("exact", [False, True], ids=["split-f16", "x3_disabled"])
@pytest.mark.parametrize("head", ["linear", "mlp"])
def test_toy_trunk_and_heads(head, exact):
    _run("toy", head, exact)


@pytest.mark.parametrize("exact", [False, True], ids=["split-f16", "x3_disabled"])
def test_one_block_per_stage_at_the_large_models_widths(exact):
    _run("wide", "mlp", exact)


def test_encode_text_on_the_gpu():
    ours = case("toy", "linear")[0]
    lit = K.LitCLIP(**K.toy_model_cfg("linear"))
    lit.load_state_dict({k: v.cpu() for k, v in ours.clip_model.state_dict().items()})
    tokens = K.toy_tokens()
    with torch.no_grad():
        want32, want64 = lit.encode_text(tokens), copy.deepcopy(lit).double().encode_text(tokens)
        got = ours.encode_text(tokens.to(DEV))
    check_4x({"text": got}, {"text": want32}, {"text": want64}, "encode_text ")
