"""MinVIS_OV on the GPU against golden g23 — the reference's own MinVIS_OV forward on its own CLIP backbone
(tests/golden/gen_minvis_ov_golden.py) — at the project's parity bar, with ENSEMBLE_ON_VALID_MASK off and on."""
import pytest
import torch

import minvis_ov_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(rtol=1e-3, atol=1e-3)         # the project's parity bar (tests/test_golden_gpu.py)


@pytest.mark.parametrize("flag", [False, True], ids=["plain", "ENSEMBLE_ON_VALID_MASK"])
def test_forward_against_the_references(flag):
    model, g, meta = M.build(flag, DEV)
    out, stages = M.run(model, g, meta, DEV)
    tag = "valid" if flag else "plain"
    for k in ("pooled_clip_feature", "out_vocab_logits", "pred_logits", "cls"):
        want = torch.from_numpy(g.z[f"{tag}/" + {"cls": "post_logits"}.get(k, k)].copy())
        print(f"{tag} {k}: max |diff| {(stages[k].cpu() - want).abs().max().item():.3e} (max |value| {want.abs().max().item():.3f})")
    M.check_against_golden(stages, g, tag, TOL)
    assert len(out["pred_scores"]) == 10 and out["pred_masks"][0].shape == (meta["T"], *meta["out_hw"])


def test_two_calls_give_the_same_results():
    model, g, meta = M.build(True, DEV)
    a, sa = M.run(model, g, meta, DEV)
    b, sb = M.run(model, g, meta, DEV)
    assert torch.equal(sa["pred_logits"], sb["pred_logits"]) and torch.equal(sa["cls"], sb["cls"])
    assert a["pred_scores"] == b["pred_scores"] and a["pred_labels"] == b["pred_labels"]
