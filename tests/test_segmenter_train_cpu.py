"""Segmenter training on CPU tensors (host logic and the torch formulations): golden g18 — the reference's own
MSDeformAttnPixelDecoder in .train() — against the package's `_train_features`, Fn.msda_fused on CPU tensors, the ResNet under
autograd on live weights, and the MinVIS stage."""
import os

import pytest
import torch
import torch.nn.functional as F

from segmenter_train_cases import G18, fused_torch, make_fused_inputs, minvis_batch, minvis_model
from test_tracker_train_gpu import TIGHT, TOL


@pytest.fixture(scope="module")
def g18():
    return G18()


def test_g18_training_step_vs_reference(g18):
    meta = g18.meta
    assert meta["smallest_distance_to_integer"] >= meta["margin"] == 5e-5
    assert meta["largest_fp32_fp64_coordinate_diff"] <= meta["margin"] / 10
    pd, outs, grads = g18.run()
    assert pd.training
    want = g18.golden_grads()
    assert set(outs) == set(g18.outs) and set(grads) == set(want)
    for tol in (TOL, TIGHT):
        for n, v in outs.items():
            torch.testing.assert_close(v, g18.outs[n], **tol, msg=lambda m, n=n: f"{n}: {m}")
        for n, g in grads.items():
            torch.testing.assert_close(g, want[n], **tol, msg=lambda m, n=n: f"{n}: {m}")


def test_g18_float64_module_stays_float64(g18):
    pd, outs, grads = g18.run(dtype=torch.float64)
    assert all(v.dtype == torch.float64 for v in outs.values()) and all(g.dtype == torch.float64 for g in grads.values())
    want = g18.golden_grads()
    for n, g in grads.items():
        torch.testing.assert_close(g.float(), want[n], **TOL, msg=lambda m, n=n: f"{n}: {m}")


def test_training_maps_are_plain_tensors_and_eval_is_untouched(g18):
    from dvis_plus_amd.pixel_decoder import TokenMaps
    pd, _, _ = g18.run()
    feats = {k: v.clone() for k, v in g18.feats.items()}
    mf, out0, ms = pd.forward_features(feats)
    assert isinstance(ms, (list, TokenMaps)) and getattr(ms, "tokens", None) is None and len(ms) == 3
    assert mf.requires_grad and out0 is ms[0]
    pd.eval()
    with torch.no_grad():
        mf_e, _, ms_e = pd.forward_features(feats)
    torch.testing.assert_close(mf_e, mf.detach(), **TIGHT)
    for a, b in zip(ms_e, ms):
        torch.testing.assert_close(a, b.detach(), **TIGHT)


@pytest.mark.parametrize("L", [1, 3])
def test_msda_fused_on_cpu_tensors_is_the_unfused_math(L):
    from dvis_plus_amd import functions as Fn
    shapes = [(3, 2), (2, 2), (2, 3)][:L]
    value, s, lsi, ref, off, lg, _ = make_fused_inputs(1, 2, 32, shapes, 3, seed=L, margin=1e-2)
    want, _, _ = fused_torch(value, s, ref, off, lg, L, 4)
    got = Fn.msda_fused(value, s, lsi, ref, off, lg, L, 4)
    assert torch.equal(got, want)
    with pytest.raises(RuntimeError, match="reference"):
        Fn.msda_fused(value, s, lsi, ref.clone().requires_grad_(), off, lg, L, 4)
    v, o, l_ = (t.double().requires_grad_() for t in (value, off, lg))
    assert torch.autograd.gradcheck(lambda a, b, c: Fn.msda_fused(a, s, lsi, ref.double(), b, c, L, 4), (v, o, l_),
                                    eps=1e-6, atol=1e-5, rtol=1e-4)


# ---- ResNet under autograd
def _resnet_restatement(m, x):
    """The backbone restated in fp64: plain conv2d + the FrozenBN affine, ReLU, the stem's max-pool, residual adds."""
    def cb(c, t):
        n = c.norm
        scale = n.weight.double() * (n.running_var.double() + n.eps).rsqrt()
        shift = n.bias.double() - n.running_mean.double() * scale
        y = F.conv2d(t, c.weight64, None, c.stride, c.padding)
        return y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    t = F.max_pool2d(F.relu(cb(m.stem.conv1, x)), 3, 2, 1)
    out = {}
    for name in m.stage_names:
        for b in getattr(m, name):
            y = F.relu(cb(b.conv2, F.relu(cb(b.conv1, t))))
            t = F.relu(cb(b.conv3, y) + (t if b.shortcut is None else cb(b.shortcut, t)))
        out[name] = t
    return out


def _randomise_frozen_bn(m, seed):
    g = torch.Generator().manual_seed(seed)
    from dvis_plus_amd.backbone import FrozenBatchNorm2d
    for mod in m.modules():
        if isinstance(mod, FrozenBatchNorm2d):
            mod.weight.copy_(0.5 + torch.rand(mod.weight.shape, generator=g))
            mod.bias.copy_(0.2 * torch.randn(mod.bias.shape, generator=g))
            mod.running_mean.copy_(0.2 * torch.randn(mod.bias.shape, generator=g))
            mod.running_var.copy_(0.5 + torch.rand(mod.bias.shape, generator=g))


def test_resnet_under_grad_reaches_every_parameter():
    from dvis_plus_amd.backbone import ConvBN, build_resnet50
    torch.manual_seed(5)
    m = build_resnet50().eval()
    _randomise_frozen_bn(m, 6)
    x = torch.randn(1, 3, 32, 32)
    xg = x.clone().requires_grad_()
    out = m(xg)
    g = torch.Generator().manual_seed(7)
    cots = {k: torch.randn(v.shape, generator=g) for k, v in out.items()}
    sum((out[k] * cots[k]).sum() / out[k].numel() for k in out).backward()
    # the fp64 restatement
    convs = [c for c in m.modules() if isinstance(c, ConvBN)]
    for c in convs:
        c.weight64 = c.weight.detach().double().requires_grad_()
    x64 = x.double().requires_grad_()
    ref = _resnet_restatement(m, x64)
    sum((ref[k] * cots[k].double()).sum() / ref[k].numel() for k in ref).backward()
    for k in out:
        torch.testing.assert_close(out[k].detach().double(), ref[k].detach(), **TOL)
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
    for c in convs:
        torch.testing.assert_close(c.weight.grad.double(), c.weight64.grad, **TOL)
    torch.testing.assert_close(xg.grad.double(), x64.grad, **TOL)


def test_resnet_with_frozen_parameters_takes_the_eval_path():
    from dvis_plus_amd.backbone import build_resnet50
    torch.manual_seed(8)
    m = build_resnet50().eval()
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        want = m(x)
    for p in m.parameters():
        p.requires_grad_(False)
    got = m(x)                                                  # grad enabled, nothing to train: today's folded path
    assert all(torch.equal(got[k], want[k]) and not got[k].requires_grad for k in want)
    next(m.parameters()).requires_grad_(True)
    live = m(x)
    assert all(v.requires_grad for v in live.values())


# ---- the MinVIS stage
def _hand_composed(m, batch, seed):
    images, _ = m.preprocess([f for v in batch for f in v["image"]])
    outputs = m.sem_seg_head(m.backbone(images))
    targets = m.prepare_targets(batch, images)
    outputs, targets = m.frame_decoder_loss_reshape(outputs, targets)
    torch.manual_seed(seed)
    losses = m.criterion(outputs, targets)
    w = m.criterion.weight_dict
    return {k: v * w[k] for k, v in losses.items() if k in w}, targets


def test_minvis_stage():
    m, wd = minvis_model()
    batch = minvis_batch()
    m.train()
    torch.manual_seed(3)
    losses = m(batch)
    assert set(losses) == set(wd) and all(torch.isfinite(v).all() for v in losses.values())
    want, targets = _hand_composed(m, batch, 3)
    assert len(targets) == 4 and all(t["ids"].shape == (2, 1) and t["masks"].shape == (2, 1, 64, 96) for t in targets)
    assert [t["ids"][:, 0].tolist() for t in targets] == [[0, -1], [0, 1]] * 2       # the instance absent everywhere is dropped
    for k in wd:
        assert torch.equal(losses[k], want[k]), k
    sum(losses.values()).backward()
    for name, mod in (("backbone", m.backbone), ("pixel_decoder", m.sem_seg_head.pixel_decoder), ("decoder", m.sem_seg_head.predictor)):
        for n, p in mod.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), (name, n)
    crit, m.criterion = m.criterion, None
    with pytest.raises(RuntimeError, match="criterion"):
        m(batch)
    m.criterion = crit
    uneven = [dict(batch[0]), dict(batch[1], image=[f[:, :32] for f in batch[1]["image"]])]
    with pytest.raises(ValueError, match="one size"):
        m(uneven)


def test_minvis_eval_is_unchanged_by_a_training_call():
    from tracker_train_cases import same_output
    m, _ = minvis_model()
    video = [{k: v for k, v in minvis_batch()[0].items() if k != "instances"}]
    before = m(video)
    m.train()
    torch.manual_seed(3)
    sum(m(minvis_batch()).values()).backward()
    m.eval()
    assert same_output(m(video), before)


def test_minvis_from_config_builds_the_criterion():
    import json
    from dvis_plus_amd.config import get_default_cfg
    from dvis_plus_amd.criterion import VideoSetCriterion
    from dvis_plus_amd.meta_architecture import MinVIS
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "cfg_MinVIS_R50.json")) as f:
        cfg = get_default_cfg().merge(json.load(f))
    ret = MinVIS.from_config(cfg)
    assert isinstance(ret["criterion"], VideoSetCriterion)
    with open(os.path.join(golden, "criterion_weight_dicts.json")) as f:
        assert ret["criterion"].weight_dict == json.load(f)["MinVIS_R50"]["weight_dict"]
