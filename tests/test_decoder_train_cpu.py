"""The masked-attention decoders under .train() on CPU tensors (torch formulations of the attention and the mask logits), against
golden g17 — the reference's own VideoMultiScaleMaskedTransformerDecoder_dvisPlus in training mode — and the output contract of all
four registered classes.

The g17 loss divides every cotangent by its prediction's number of elements, so most gradients are smaller than TIGHT's atol; each
gradient is therefore also held to TIGHT's rtol at its tensor's own scale (max |recorded gradient|)."""
import pytest
import torch

from decoder_train_cases import G17, build_decoder, check_predictions, golden_grads, train_run
from test_tracker_train_gpu import TIGHT, TOL

CLASSES = ["MultiScaleMaskedTransformerDecoder", "VideoMultiScaleMaskedTransformerDecoder_dvisPlus",
           "VideoMultiScaleMaskedTransformerDecoder_dvis", "VideoMultiScaleMaskedTransformerDecoder_minvis"]


@pytest.fixture(scope="module")
def g17():
    return G17()


def test_fixture_condition(g17):
    assert g17.meta["smallest_abs_downsized_logit"] >= 1e-4
    assert g17.meta["levels"] == ((3, 6), (6, 12), (12, 24)) and g17.meta["layers"] == 4


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_training_step_vs_reference(g17, dtype):
    dec, out, masks, grads = train_run(g17, "cpu", dtype)
    L = g17.meta["layers"]
    assert len(out["aux_outputs"]) == L and len(masks) == L
    for i, (got, want) in enumerate(zip(masks, g17.masks())):
        assert torch.equal(got, want), f"layer {i}: effective attention mask differs from the recording"
    check_predictions(g17, out, (TOL, TIGHT))
    want = golden_grads(g17)
    assert set(want) == set(grads)
    for tol in (TOL, TIGHT):
        for n, w in want.items():
            torch.testing.assert_close(grads[n].float(), w, **tol, msg=lambda m, n=n: f"{n}: {m}")
    worst = 0.0
    for n, w in want.items():
        err, scale = (grads[n].double() - w.double()).abs().max().item(), w.abs().max().item()
        worst = max(worst, err / scale)
        assert err <= TIGHT["rtol"] * scale, (n, err, scale)
    print(f"{dtype}: worst gradient error relative to its tensor's scale {worst:.3e}")


def test_loss_matches_the_recording(g17):
    from decoder_train_cases import loss_of
    dec = build_decoder(g17).train()
    x, mf = g17.inputs()
    loss = loss_of(dec(x, mf), g17.cot(), g17.meta["hidden"])
    torch.testing.assert_close(loss.detach(), g17.t("loss"), rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("cls", CLASSES)
def test_shapes_and_keys_under_train_and_eval_afterwards(g17, cls):
    m = g17.meta
    dec = build_decoder(g17, cls=cls).train()
    x, mf = g17.inputs()
    out = dec(x, mf)
    N, Q, K1, C, L, H, W = 4, m["Q"], m["classes"] + 1, m["hidden"], m["layers"], m["H"], m["W"]
    b, t = N // m["num_frames"], m["num_frames"]
    video = cls != "MultiScaleMaskedTransformerDecoder"
    logits_shape = (b, t, Q, K1) if video else (N, Q, K1)
    masks_shape = (b, Q, t, H, W) if video else (N, Q, H, W)
    keys = {"pred_logits", "pred_masks", "aux_outputs"}
    if video:
        keys |= {"pred_embds", "pred_embds_without_norm"}
        if not cls.endswith("minvis"):
            keys.add("mask_features")
    width = C
    if cls.endswith("dvisPlus"):
        keys.add("pred_reid_embed")
        width = 2 * C
        assert out["pred_reid_embed"].shape == (b, C, t, Q)
    assert set(out) == keys
    assert out["pred_logits"].shape == logits_shape and out["pred_masks"].shape == masks_shape
    assert len(out["aux_outputs"]) == L
    for a in out["aux_outputs"]:
        assert set(a) == {"pred_logits", "pred_masks"}
        assert a["pred_logits"].shape == logits_shape and a["pred_masks"].shape == masks_shape
        assert a["pred_logits"].requires_grad and a["pred_masks"].requires_grad
    if video:
        assert out["pred_embds"].shape == out["pred_embds_without_norm"].shape == (b, width, t, Q)
    # all four classes compute the same L + 1 predictions from the same weights
    want = g17.t(f"{L}/pred_masks", g17.preds)
    got = out["pred_masks"] if video else out["pred_masks"].unflatten(0, (b, t)).transpose(1, 2)
    torch.testing.assert_close(got.detach(), want, **TIGHT)
    dec.eval()
    with torch.no_grad():
        ev = dec(x, mf)
    assert ev["aux_outputs"] == []
    assert all(not v.requires_grad for v in ev.values() if torch.is_tensor(v))
    if video:                                              # eval: all frames form one clip
        assert ev["pred_logits"].shape == (1, N, Q, K1) and ev["pred_masks"].shape == (1, Q, N, H, W)


@pytest.mark.parametrize("cls", CLASSES[1:])
def test_frames_must_be_a_multiple_of_num_frames(g17, cls):
    dec = build_decoder(g17, cls=cls).train()
    x, mf = g17.inputs()
    with pytest.raises(ValueError, match="num_frames"):
        dec([t[:3] for t in x], mf[:3])
    dec.eval()
    with torch.no_grad():
        assert dec([t[:3] for t in x], mf[:3])["pred_logits"].shape[1] == 3


def test_mask_features_without_grad_take_the_single_mask_logits_call(g17, monkeypatch):
    from dvis_plus_amd import functions as Fn
    calls = []
    orig = Fn.mask_logits
    monkeypatch.setattr(Fn, "mask_logits", lambda e, f: calls.append(e.shape[1]) or orig(e, f))
    _, out, _, grads = train_run(g17, "cpu", features_grad=False)
    Q, L = g17.meta["Q"], g17.meta["layers"]
    assert calls == [(L + 1) * Q]
    want = golden_grads(g17)
    for n in grads:
        torch.testing.assert_close(grads[n], want[n], **TIGHT, msg=lambda m, n=n: f"{n}: {m}")
    calls.clear()
    train_run(g17, "cpu", features_grad=True)
    assert calls == [Q] * (L + 1)
