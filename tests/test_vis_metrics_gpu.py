"""GPU: the VIS kernels (csrc/vis_metrics.hip) equal their CPU formulations exactly, and YTVISEvaluator fed device outputs
reproduces the reference's VIS evaluation (fixture g12) — result dict and results.json bytes."""
import json

import pytest
import torch

from dvis_plus_amd import cpu_ops
from dvis_plus_amd import functions as Fn
import test_vis_metrics_cpu as C
from test_vis_metrics_cpu import g12  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def blocky(N, H, W, seed, block=(40, 64), p=0.4):
    """(N, H, W) bool masks made of blocks (COCO runs of realistic length), with the fixture's edge cases in the first three."""
    g = torch.Generator().manual_seed(seed)
    bh, bw = block
    cells = torch.rand((N, (H + bh - 1) // bh + 1, (W + bw - 1) // bw + 1), generator=g) < p
    m = cells.repeat_interleave(bh, 1).repeat_interleave(bw, 2)[:, :H, :W].contiguous()
    if N >= 3:
        m[0, 0, 0] = True                 # pixel (0, 0): a leading empty run
        m[1] = True                       # all ones
        m[2, :, : min(W, 5)] = True       # full columns: runs across the column wrap
    return m


def check_codec(m):
    N, H, W = m.shape
    ref = cpu_ops.rle_encode(m)
    got = Fn.rle_encode(m.to(DEV))
    for a, b in zip(ref, got):
        assert torch.equal(a, b.cpu())
    s_ref = cpu_ops.rle_strings(ref[0], ref[1])
    s_got = Fn.rle_strings(got[0], got[1])
    for a, b in zip(s_ref, s_got):
        assert torch.equal(a, b.cpu())
    assert torch.equal(Fn.rle_decode(got[0], got[1], H, W).cpu(), cpu_ops.rle_decode(ref[0], ref[1], H, W))


@pytest.mark.parametrize("shape", [(5, 7, 9), (3, 37, 53), (4, 33, 65), (3, 1, 5), (3, 5, 1), (3, 24, 40), (2, 272, 480)])
def test_codec_edge_shapes(shape):
    """W not a multiple of 4 or 64, H * W not a multiple of 64, single rows / columns, byte and word load paths."""
    check_codec(blocky(*shape, seed=sum(shape), block=(3, 4)))


def test_codec_and_intersections_on_the_fixture(g12):
    for vid in g12["video_ids"]:
        _, out = C.video_outputs(g12, int(vid))
        m = out["pred_masks"]
        P, T, H, W = m.shape
        if P == 0:
            continue
        check_codec(m.reshape(P * T, H, W))
        gt = m.flip(0)[: max(1, P // 2)]
        ref = cpu_ops.track_intersections(m, gt)
        assert torch.equal(Fn.track_intersections(m.to(DEV), gt.to(DEV)).cpu(), ref)


def test_kernels_on_a_720p_video():
    """YTVIS shape: 720p, T = 36, P = 10 predicted and G = 6 ground-truth tracks; intersections also in two frame chunks."""
    P, G, T, H, W = 10, 6, 36, 720, 1280
    pred = blocky(P * T, H, W, seed=1).view(P, T, H, W)
    gt = blocky(G * T, H, W, seed=2, block=(48, 80)).view(G, T, H, W)
    check_codec(pred[:2].reshape(2 * T, H, W))
    ref = cpu_ops.track_intersections(pred, gt)
    pd, gd = pred.to(DEV), gt.to(DEV)
    assert torch.equal(Fn.track_intersections(pd, gd).cpu(), ref)
    acc = Fn.track_intersections(pd[:, :20], gd[:, :20])
    Fn.track_intersections(pd[:, 20:], gd[:, 20:], out=acc)
    assert torch.equal(acc.cpu(), ref)


def test_intersections_many_tracks_split_over_launches():
    """P = 100 predicted tracks and G = 120 ground-truth tracks do not fit one launch's LDS: the table is built in column slices."""
    P, G, T, H, W = 100, 120, 2, 40, 72
    pred = blocky(P * T, H, W, seed=5, block=(4, 6)).view(P, T, H, W)
    gt = blocky(G * T, H, W, seed=6, block=(5, 4)).view(G, T, H, W)
    assert torch.equal(Fn.track_intersections(pred.to(DEV), gt.to(DEV)).cpu(), cpu_ops.track_intersections(pred, gt))


def test_evaluator_on_device_outputs_reproduces_the_reference(g12, tmp_path):
    """Two runs of the same evaluator give identical results (integer counting only); both equal the fixture."""
    want = json.loads(C.text(g12, "results_dict"))["segm"]
    for i in range(2):
        ev = C.make_evaluator(g12, str(tmp_path / f"run{i}"))
        res = C.run(g12, ev, device=DEV)
        C.same_results(res["segm"], want)
        with open(tmp_path / f"run{i}" / "out" / "results.json") as f:
            assert f.read() == C.text(g12, "results_json")
        assert all(v[2] is not None for v in ev._videos)


def test_command_line_on_the_device(g12, tmp_path):
    gt = tmp_path / "instances.json"
    gt.write_text(C.text(g12, "gt_json"))
    res = tmp_path / "results.json"
    res.write_text(C.text(g12, "results_json"))
    from dvis_plus_amd import vis_metrics as VIS
    C.same_results(VIS.main(["--gt", str(gt), "--results", str(res)]), json.loads(C.text(g12, "results_dict"))["segm"])
