"""GPU: the video-metric kernels (csrc/video_metrics.hip) equal the bincount formulation exactly, and the metrics computed from
them equal the reference scripts' numbers (fixture g11)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

from dvis_plus_amd import functions as Fn
from dvis_plus_amd import video_metrics as VM
import test_video_metrics_cpu as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g11():
    return np.load(os.path.join(GOLDEN, "g11_video_metrics.npz"))


def blocky(T, H, W, n, seed, block=(40, 64)):
    """(T, H, W) int32 map of n ids in blocks that shift with t."""
    g = torch.Generator().manual_seed(seed)
    bh, bw = block
    cells = torch.randint(0, n, (T, (H + bh - 1) // bh + 1, (W + bw - 1) // bw + 1), generator=g, dtype=torch.int32)
    cells[1:] = torch.where(torch.rand(cells[1:].shape, generator=g) < 0.8, cells[:1].expand_as(cells[1:]), cells[1:])
    m = cells.repeat_interleave(bh, 1).repeat_interleave(bw, 2)
    return m[:, :H, :W].contiguous()


def check_all(gt, pred, table, num_pred, nc=124, ks=(8, 16)):
    h_ref = Fn.pan_pair_hist(gt, pred, table, num_pred)
    h = Fn.pan_pair_hist(gt.to(DEV), pred.to(DEV), table.to(DEV), num_pred)
    assert torch.equal(h.cpu(), h_ref)
    sg, sp = gt % 256, pred % 256
    c_ref = Fn.sem_confusion(sg, sp % nc, nc)
    assert torch.equal(Fn.sem_confusion(sg.to(DEV), (sp % nc).to(DEV), nc).cpu(), c_ref)
    v_ref = Fn.video_consistency(sg, sp, ks)
    v = Fn.video_consistency(sg.to(DEV), sp.to(DEV), ks)
    assert torch.equal(v[0].cpu(), v_ref[0]) and torch.equal(v[1].cpu(), v_ref[1])
    return h


def test_kernels_equal_the_cpu_formulation_on_the_fixture(g11):
    gj, pa, ga = C._vipseg(g11)
    for v in gj["videos"]:
        vid = v["video_id"]
        gt = VM.PanopticGT(ga[vid])
        pred, table = VM.PanopticPred.from_json(pa[vid])
        pm = VM.map_pred_ids(torch.from_numpy(g11[f"vipseg/{vid}/pred"]), table, True)
        check_all(torch.from_numpy(g11[f"vipseg/{vid}/gt"]), pm, torch.as_tensor(gt.table), pred.num_pred)
    for vid in g11["vspw/videos"]:
        g = torch.from_numpy(g11[f"vspw/{vid}/gt"].astype(np.int32))
        p = torch.from_numpy(g11[f"vspw/{vid}/pred"].astype(np.int32))
        assert torch.equal(Fn.sem_confusion(g.to(DEV), p.to(DEV), 124).cpu(), Fn.sem_confusion(g, p, 124))


def test_random_blocky_720p_clip():
    T, H, W = 30, 720, 1280
    table = torch.arange(1, 41, dtype=torch.int32) * 1000 + 7
    gt = table[blocky(T, H, W, 40, 0).long()]
    gt[:, :8] = 0                                     # VOID
    gt[:, -5:, :9] = 123                              # not in the table
    pred = blocky(T, H, W, 31, 1, (36, 80))
    check_all(gt, pred, table, 30)


def test_global_atomic_fallback_past_the_lds_budget():
    T, H, W = 3, 97, 131
    table = torch.arange(1, 301, dtype=torch.int32) * 3
    gt = table[blocky(T, H, W, 300, 2, (3, 5)).long()]
    pred = blocky(T, H, W, 101, 3, (4, 3))
    assert (300 + 2) * 101 * 4 > 64 * 1024
    check_all(gt, pred, table, 100)
    check_all(gt % 250, pred, torch.arange(1, 250, dtype=torch.int32), 100, nc=200)      # 200 x 200 confusion: global path


def test_short_clips_and_odd_sizes():
    table = torch.tensor([2, 5, 9], dtype=torch.int32)
    for T, H, W in ((1, 17, 23), (5, 33, 7), (9, 3, 1001), (16, 11, 13), (17, 1, 1)):
        gt = table[blocky(T, H, W, 3, T, (2, 3)).long()]
        check_all(gt, blocky(T, H, W, 4, T + 1, (3, 2)), table, 3)


def test_non_contiguous_inputs_work():
    table = torch.tensor([2, 5, 9], dtype=torch.int32)
    gt = table[blocky(10, 40, 64, 3, 4).long()].to(DEV)
    pred = blocky(10, 40, 64, 4, 5).to(DEV)
    h = Fn.pan_pair_hist(gt.transpose(1, 2), pred.transpose(1, 2), table.to(DEV), 3)
    assert torch.equal(h, Fn.pan_pair_hist(gt, pred, table.to(DEV), 3))
    v = Fn.video_consistency(gt[:, ::2], pred[:, ::2].long())
    r = Fn.video_consistency(gt[:, ::2].cpu(), pred[:, ::2].cpu())
    assert torch.equal(v[0].cpu(), r[0]) and torch.equal(v[1].cpu(), r[1])


def test_gpu_metrics_equal_the_reference_and_runs_are_bit_identical(g11):
    a = C.vipseg_scores(g11, DEV), C.vspw_scores(g11, DEV)
    C.check_vipseg(g11, *a[0])
    C.check_vspw(g11, *a[1])
    b = C.vipseg_scores(g11, DEV), C.vspw_scores(g11, DEV)
    assert a[0][0]["vpq_all"] == b[0][0]["vpq_all"] and a[0][1]["STQ"] == b[0][1]["STQ"]
    assert a[1][0]["mIoU"] == b[1][0]["mIoU"] and a[1][1]["VC16"] == b[1][1]["VC16"]
    T, H, W = 30, 720, 1280
    gt, pred = blocky(T, H, W, 40, 7).to(DEV) + 1, blocky(T, H, W, 30, 8).to(DEV)
    table = torch.arange(1, 41, dtype=torch.int32, device=DEV)
    assert torch.equal(Fn.pan_pair_hist(gt, pred, table, 29), Fn.pan_pair_hist(gt, pred, table, 29))


def test_end_to_end_product_outputs_through_the_evaluators(tmp_path):
    """A small product model in VPS and VSS mode (smoke()'s 128 x 256 shape) -> the evaluators on the device == the same
    evaluators fed the same maps on the CPU."""
    import json
    from PIL import Image
    from dvis_plus_amd.evaluation import VPSEvaluator, VSSEvaluator
    from dvis_plus_amd.meta_architecture import build_dvis_plus_r50
    H, W, T = 128, 256, 3
    gg = torch.Generator().manual_seed(1)
    frames = [torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=gg) for _ in range(T)]
    names = [f"{t:05d}" for t in range(T)]
    inputs = [{"image": [f.to(DEV) for f in frames], "height": H, "width": W, "video_id": "v0",
               "file_names": [n + ".jpg" for n in names], "frame_idx": list(range(T))}]
    results = {}
    for task in ("vps", "vss"):
        m = build_dvis_plus_r50("offline", task=task, num_classes=20, n_things=10, enc_layers=1, dec_layers=3,
                                tracker_layers=1, refiner_layers=1, max_num=10, object_mask_threshold=0.0).to(DEV)
        with torch.no_grad():
            results[task] = m(inputs)
    # ground truth: blocky maps with the ids / classes the outputs use
    root = str(tmp_path)
    gt_ids = blocky(T, H, W, 4, 9, (32, 64)) * 1000 + 70000
    gt_ids[:, :4] = 0
    cats = [{"id": i, "isthing": int(i < 10)} for i in range(20)]
    anns = []
    os.makedirs(os.path.join(root, "pan", "v0"))
    for t in range(T):
        ids = torch.unique(gt_ids[t]).tolist()
        anns.append({"file_name": names[t] + ".png", "segments_info": [
            {"id": i, "category_id": (i // 1000) % 20, "iscrowd": 0, "area": int((gt_ids[t] == i).sum())} for i in ids if i]})
        a = gt_ids[t].numpy().astype(np.int64)
        Image.fromarray(np.stack([a % 256, a // 256 % 256, a // 65536], -1).astype(np.uint8)).save(
            os.path.join(root, "pan", "v0", names[t] + ".png"))
    with open(os.path.join(root, "gt.json"), "w") as f:
        json.dump({"categories": cats, "videos": [{"video_id": "v0", "images": [{"file_name": n + ".png"} for n in names]}],
                   "annotations": [{"video_id": "v0", "annotations": anns}]}, f)
    vspw = os.path.join(root, "VSPW")
    os.makedirs(os.path.join(vspw, "data", "v0", "mask"))
    for t in range(T):
        Image.fromarray((blocky(1, H, W, 21, 10 + t)[0] % 21).numpy().astype(np.uint8)).save(
            os.path.join(vspw, "data", "v0", "mask", names[t] + ".png"))
    got = {}
    for dev in (DEV, "cpu"):
        vps = VPSEvaluator("x", None, True, None, panoptic_root=os.path.join(root, "pan"),
                           panoptic_json=os.path.join(root, "gt.json"), thing_dataset_ids=list(range(10)),
                           stuff_dataset_ids=list(range(10, 20)), device=dev)
        vss = VSSEvaluator("x", None, True, None, vspw_root=vspw, dataset_ids=list(range(20)), ignore_label=255, device=dev,
                           ks=(1, 2))
        vps.reset()
        vss.reset()
        out_vps, out_vss = dict(results["vps"]), dict(results["vss"])
        if dev == "cpu":
            out_vps["pred_masks"], out_vss["pred_masks"] = out_vps["pred_masks"].cpu(), out_vss["pred_masks"].cpu()
        vps.process(inputs, out_vps)
        vss.process(inputs, out_vss)
        got[dev] = (vps.evaluate(), vss.evaluate())
    assert results["vps"]["pred_masks"].is_cuda and len(results["vps"]["segments_infos"]) > 0
    a, b = got[DEV], got["cpu"]
    assert a[0]["vpq"]["vpq_all"] == b[0]["vpq"]["vpq_all"] and a[0]["vpq"]["per_nframes"][1] == b[0]["vpq"]["per_nframes"][1]
    assert a[0]["stq"]["STQ"] == b[0]["stq"]["STQ"] or (np.isnan(a[0]["stq"]["STQ"]) and np.isnan(b[0]["stq"]["STQ"]))
    for k, v in a[1]["sem_seg"].items():
        assert v == b[1]["sem_seg"][k] or (np.isnan(v) and np.isnan(b[1]["sem_seg"][k])), k
