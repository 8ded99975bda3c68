"""The Swin backbone on the GPU: both g21 fixtures (the reference's own D2SwinTransformer) at the project's parity bar, and a toy
DVIS_Plus_online built from a cfg with ``BACKBONE.NAME: D2SwinTransformer`` — against CPU tensors, replayed from the captured
segmenter graph, and one training step of the tracker stage on the frozen backbone."""
import pytest
import torch

import swin_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(rtol=1e-3, atol=1e-3)         # the project's parity bar (tests/test_golden_gpu.py)


@pytest.mark.parametrize("name", S.FIXTURES)
def test_fixture(name):
    fx = S.fixture(name)
    got = S.run_with_blocks(fx.build(DEV), fx.image.to(DEV))
    assert sorted(got) == sorted(fx.outs)
    for k, want in fx.outs.items():
        g = got[k].cpu()
        print(f"{name} {k}: max |diff| {(g - want).abs().max().item():.3e} (max |value| {fx.meta['max_abs'][k]:.3f})")
    for k, want in fx.outs.items():
        assert got[k].is_contiguous()
        torch.testing.assert_close(got[k].cpu(), want, **TOL)


def _continuous(m, video):
    """The segmenter's per-frame queries, logits and mask features, and the model's sorted scores."""
    with torch.no_grad():
        images, _ = m.preprocess(video["image"])
        seg = [t.float().cpu() for t in m.segment(images)]
        out = m([video])
    return seg + [torch.tensor(sorted(out["pred_scores"]))]


def test_online_model_vs_cpu_tensors():
    video = S.toy_video()
    want = _continuous(S.toy_online_model("cpu"), video)
    got = _continuous(S.toy_online_model(DEV), video)
    for i, (g, w) in enumerate(zip(got, want)):
        print(f"output {i} {tuple(w.shape)}: max |diff| {(g - w).abs().max().item():.3e} (max |value| {w.abs().max().item():.3f})")
    for g, w in zip(got, want):
        torch.testing.assert_close(g, w, **TOL)


def test_online_segmenter_graph_replay_equals_eager(monkeypatch):
    m = S.toy_online_model(DEV)
    videos = [S.toy_video(seed=1), S.toy_video(seed=2)]

    def run():
        outs = []
        for v in videos:
            o = m([v])
            outs.append(([x.clone() for x in o["pred_masks"]], list(o["pred_scores"]), list(o["pred_labels"])))
        return outs
    monkeypatch.setenv("DVIS_SEGMENTER_GRAPH", "0")
    eager = run()
    assert m._seg_graph is None or not m._seg_graph._cache
    monkeypatch.setenv("DVIS_SEGMENTER_GRAPH", "8")
    first, replay = run(), run()                    # capture (first call of the shape), then replays
    assert len(m._seg_graph._cache) == 1
    for a, b, c in zip(eager, first, replay):
        assert a[1] == b[1] == c[1] and a[2] == b[2] == c[2]
        assert len(a[0]) == len(b[0]) == len(c[0]) > 0
        assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a[0], b[0], c[0]))


def test_online_model_training_step_on_the_frozen_backbone():
    m = S.toy_online_model(DEV).train()
    losses = m([S.toy_video(instances=True)])
    assert losses and all(torch.isfinite(v).all() for v in losses.values())
    sum(losses.values()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.tracker.parameters())
    assert all(p.grad is None for mod in (m.backbone, m.sem_seg_head) for p in mod.parameters())
