"""CPU: the video metrics (dvis_plus_amd.video_metrics / evaluation) against the reference scripts' own numbers (fixture g11,
tests/golden/gen_metrics_golden.py) — counts by the bincount formulation, everything after them as on the GPU path."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

from dvis_plus_amd import functions as Fn
from dvis_plus_amd import video_metrics as VM

NF = VM.VPQ_NFRAMES


@pytest.fixture(scope="module")
def g11():
    return np.load(os.path.join(GOLDEN, "g11_video_metrics.npz"))


def _vipseg(z):
    gj, pj = json.loads(str(z["vipseg/gt_json"])), json.loads(str(z["vipseg/pred_json"]))
    pa = {a["video_id"]: a["annotations"] for a in pj["annotations"]}
    ga = {a["video_id"]: a["annotations"] for a in gj["annotations"]}
    return gj, pa, ga


def vipseg_scores(z, device="cpu"):
    gj, pa, ga = _vipseg(z)
    vpq = VM.VPQ(gj["categories"])
    stq = VM.STQ([c["id"] for c in gj["categories"] if c["isthing"]], **VM.STQ_ARGS)
    for i, v in enumerate(gj["videos"]):
        vid = v["video_id"]
        gt = VM.PanopticGT(ga[vid])
        pred, table = VM.PanopticPred.from_json(pa[vid])
        gm = torch.from_numpy(z[f"vipseg/{vid}/gt"]).to(device)
        pm = VM.map_pred_ids(torch.from_numpy(z[f"vipseg/{vid}/pred"]).to(device), table, True)
        hist = VM.pair_hist(gm, pm, gt, pred.num_pred)
        vpq.update(None, None, gt, pred, hist=hist)
        stq.update(None, None, gt, pred, i, hist=hist)
    return vpq.result(), stq.result()


def vspw_scores(z, device="cpu"):
    sc, vc = VM.SemSegConfusion(124), VM.VideoConsistency((8, 16))
    for vid in z["vspw/videos"]:
        g = torch.from_numpy(z[f"vspw/{vid}/gt"].astype(np.int32)).to(device)
        p = torch.from_numpy(z[f"vspw/{vid}/pred"].astype(np.int32)).to(device)
        sc.update(g, p)
        vc.update(g, p)
    return sc.result(), vc.result()


def check_vipseg(z, vpq, stq):
    got = np.array([[100 * vpq["per_nframes"][nf][n]["pq"] for n in ("All", "Things", "Stuff")] for nf in NF])
    np.testing.assert_allclose(got, z["vipseg/out/vpq_per_nframes"], rtol=1e-12, atol=0)
    for nf in NF:
        table = z[f"vipseg/out/vpq_class_{nf}"]          # id, PQ, SQ, RQ, IoU, TP, FP, FN as eval_vpq_vspw.py prints them
        pc = vpq["per_nframes"][nf]["per_class"]
        assert [int(k) for k in pc] == table[:, 0].astype(int).tolist()
        mine = np.array([[pc[k]["tp"], pc[k]["fp"], pc[k]["fn"]] for k in pc])
        np.testing.assert_array_equal(mine, table[:, 5:8].astype(np.int64))
        np.testing.assert_allclose([pc[k]["iou"] for k in pc], table[:, 4], atol=0.05 + 1e-9)
    final = "vpq_all:%.4f\nvpq_thing:%.4f\nvpq_stuff:%.4f\n" % (vpq["vpq_all"], vpq["vpq_thing"], vpq["vpq_stuff"])
    assert final == str(z["vipseg/out/vpq_final_txt"])
    np.testing.assert_allclose([stq["STQ"], stq["AQ"], stq["IoU"]], z["vipseg/out/stq"], rtol=1e-12, atol=0)


def check_vspw(z, miou, vc):
    got = [miou["Acc"], miou["Acc_class"], miou["mIoU"], miou["fwIoU"]]
    np.testing.assert_allclose(got, z["vspw/out/miou"], rtol=1e-12, atol=0)
    np.testing.assert_allclose([vc["VC8"], vc["VC16"]], z["vspw/out/vc"], rtol=1e-12, atol=0)


def test_cpu_path_reproduces_the_reference_scripts(g11):
    check_vipseg(g11, *vipseg_scores(g11))
    check_vspw(g11, *vspw_scores(g11))


def test_vc_per_window_length_alone(g11):
    """VC16_k_only: the windows of length 16 only (the script's VC16 also averages the VC8 windows)."""
    accs = []
    for vid in g11["vspw/videos"]:
        g, p = g11[f"vspw/{vid}/gt"], g11[f"vspw/{vid}/pred"]
        T = len(g)
        for i in range(T - 16):
            cg = (g[i:i + 16] == g[i]).all(0)
            accs.append((cg & (p[i:i + 16] == p[i]).all(0)).sum() / cg.sum())
    _, vc = vspw_scores(g11)
    assert vc["VC16_k_only"] == pytest.approx(np.nanmean(accs), rel=1e-12)


def test_count_formulations_on_small_maps():
    g = torch.tensor([[[0, 5, 5, 9], [70000, 5, 0, 3]]], dtype=torch.int32)
    p = torch.tensor([[[0, 1, 1, 2], [2, 2, 0, 1]]], dtype=torch.int32)
    h = Fn.pan_pair_hist(g, p, torch.tensor([5, 9, 70000]), 2)
    assert h.shape == (1, 5, 3) and int(h.sum()) == 8
    assert h[0, 0, 0] == 2 and h[0, 1, 1] == 2 and h[0, 1, 2] == 1 and h[0, 2, 2] == 1 and h[0, 3, 2] == 1 and h[0, 4, 1] == 1
    with pytest.raises(ValueError):
        Fn.pan_pair_hist(g, p, torch.tensor([5, 9, 70000]), 1)
    c = Fn.sem_confusion(torch.tensor([0, 1, 2, 255, 3]), torch.tensor([0, 0, 1, 7, 2]), 3)
    assert c.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    gc, bc = Fn.video_consistency(torch.zeros(3, 2, 2, dtype=torch.int32), torch.arange(12).view(3, 2, 2), (1, 2, 3))
    assert gc.tolist() == [[4, 4, 0], [4, 0, 0], [0, 0, 0]] and bc.tolist() == [[4, 4, 0], [0, 0, 0], [0, 0, 0]]


def rebuild_trees(z, root):
    """The fixture's VIPSeg / VSPW trees on disk, as gen_metrics_golden.py laid them out."""
    from PIL import Image
    gj, pa, ga = _vipseg(z)
    truth, submit = os.path.join(root, "gt"), os.path.join(root, "submit")
    for v in gj["videos"]:
        vid = v["video_id"]
        os.makedirs(os.path.join(truth, vid))
        os.makedirs(os.path.join(submit, "pan_pred", vid))
        for t, im in enumerate(v["images"]):
            for arr, d in ((z[f"vipseg/{vid}/gt"][t], truth), (z[f"vipseg/{vid}/pred"][t], os.path.join(submit, "pan_pred"))):
                a = arr.astype(np.int64)
                Image.fromarray(np.stack([a % 256, a // 256 % 256, a // 65536], -1).astype(np.uint8)).save(
                    os.path.join(d, vid, im["file_name"]))
    with open(os.path.join(root, "gt.json"), "w") as f:
        json.dump(gj, f)
    with open(os.path.join(submit, "pred.json"), "w") as f:
        f.write(str(z["vipseg/pred_json"]))
    vspw, pred = os.path.join(root, "VSPW"), os.path.join(root, "vss_pred")
    with open(os.path.join(os.makedirs(vspw) or vspw, "val.txt"), "w") as f:
        f.write("".join(str(v) + "\n" for v in z["vspw/videos"]))
    for vid in z["vspw/videos"]:
        os.makedirs(os.path.join(vspw, "data", str(vid), "mask"))
        os.makedirs(os.path.join(pred, str(vid)))
        for t in range(len(z[f"vspw/{vid}/gt"])):
            Image.fromarray(z[f"vspw/{vid}/gt"][t]).save(os.path.join(vspw, "data", str(vid), "mask", f"{t:05d}.png"))
            Image.fromarray(z[f"vspw/{vid}/pred"][t]).save(os.path.join(pred, str(vid), f"{t:05d}.png"))
    return truth, submit, vspw, pred


def test_command_line_rescoring_an_existing_prediction_tree(g11, tmp_path, capsys):
    truth, submit, vspw, pred = rebuild_trees(g11, str(tmp_path))
    common = ["--submit_dir", submit, "--truth_dir", truth, "--pan_gt_json_file", str(tmp_path / "gt.json"), "--device", "cpu"]
    vpq = VM.main(["vpq", *common])
    stq = VM.main(["stq", *common])
    check_vipseg(g11, vpq, stq)
    assert open(os.path.join(submit, "vpq-final.txt")).read() == str(g11["vipseg/out/vpq_final_txt"])
    for nf in NF:
        assert open(os.path.join(submit, "vpq-%d.txt" % ((nf - 1) * 5))).read() == str(g11[f"vipseg/out/vpq_txt_{nf}"])
    miou = VM.main(["miou", vspw, pred, "--device", "cpu"])
    vc = VM.main(["vc", vspw, pred, "--device", "cpu"])
    check_vspw(g11, miou, vc)
    out = capsys.readouterr().out
    assert "VC16 score: {} on val.txt set".format(vc["VC16"]) in out and "STQ : {}".format(stq["STQ"]) in out


def vps_outputs(z, vid, gj, pa):
    """The fixture's predictions as the product's VPS output (dense ids 1..n in raw-id order, contiguous categories: VIPSeg's
    things first then stuff, as the dataset registration orders them)."""
    pred, table = VM.PanopticPred.from_json(pa[vid])
    dense = VM.map_pred_ids(torch.from_numpy(z[f"vipseg/{vid}/pred"]), table, True)
    things = [c["id"] for c in gj["categories"] if c["isthing"]]
    stuff = [c["id"] for c in gj["categories"] if not c["isthing"]]
    contiguous = {d: n for n, d in enumerate(things + stuff)}
    segs = [{"id": d, "isthing": int(pred.category[d]) in things, "category_id": contiguous[int(pred.category[d])]}
            for d in range(1, pred.num_pred + 1)]
    return {"image_size": tuple(dense.shape[1:]), "pred_masks": dense, "segments_infos": segs, "pred_ids": [], "task": "vps"}


def make_evaluators(z, root):
    from dvis_plus_amd.evaluation import VPSEvaluator, VSSEvaluator
    truth, _, vspw, _ = rebuild_trees(z, root)
    gj, _, _ = _vipseg(z)
    things = [c["id"] for c in gj["categories"] if c["isthing"]]
    stuff = [c["id"] for c in gj["categories"] if not c["isthing"]]
    vps = VPSEvaluator("vipseg_val", None, True, None, panoptic_root=truth, panoptic_json=os.path.join(root, "gt.json"),
                       thing_dataset_ids=things, stuff_dataset_ids=stuff, device="cpu")
    # VSPW's registration maps dataset id c <-> contiguous class c (datasets/vss.py: get_metadata)
    vss = VSSEvaluator("vspw_val", None, True, None, vspw_root=vspw, dataset_ids=list(range(124)), ignore_label=255,
                       device="cpu")
    return vps, vss


def run_evaluators(z, vps, vss, videos_vps, videos_vss):
    gj, pa, _ = _vipseg(z)
    vps.reset()
    vss.reset()
    for v in gj["videos"]:
        if v["video_id"] in videos_vps:
            inputs = [{"video_id": v["video_id"], "file_names": [f"img/{im['file_name'][:-4]}.jpg" for im in v["images"]],
                       "frame_idx": list(range(len(v["images"])))}]
            vps.process(inputs, vps_outputs(z, v["video_id"], gj, pa))
    for vid in z["vspw/videos"]:
        if str(vid) in videos_vss:
            gt = z[f"vspw/{vid}/gt"]
            sem = torch.from_numpy(z[f"vspw/{vid}/pred"].astype(np.int64))
            inputs = [{"video_id": str(vid), "file_names": [f"{t:05d}.jpg" for t in range(len(gt))],
                       "frame_idx": list(range(len(gt)))}]
            vss.process(inputs, {"image_size": gt.shape[1:], "pred_masks": sem, "task": "vss"})
    return vps.evaluate(), vss.evaluate()


def test_evaluator_protocol_on_reference_format_outputs(g11, tmp_path):
    vps, vss = make_evaluators(g11, str(tmp_path))
    gj, _, _ = _vipseg(g11)
    r_vps, r_vss = run_evaluators(g11, vps, vss, {v["video_id"] for v in gj["videos"]}, {str(v) for v in g11["vspw/videos"]})
    check_vipseg(g11, r_vps["vpq"], r_vps["stq"])
    check_vspw(g11, {k: r_vss["sem_seg"][k] for k in ("Acc", "Acc_class", "mIoU", "fwIoU")},
               {k: r_vss["sem_seg"][k] for k in ("VC8", "VC16")})


def _world2_worker(rank, root, init, outq):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=2)
    z = np.load(os.path.join(GOLDEN, "g11_video_metrics.npz"))
    vps, vss = make_evaluators(z, os.path.join(root, f"r{rank}"))
    gj, _, _ = _vipseg(z)
    mine_vps = {v["video_id"] for n, v in enumerate(gj["videos"]) if n % 2 == rank}
    mine_vss = {str(v) for n, v in enumerate(z["vspw/videos"]) if (n + 1) % 2 == rank}
    r = run_evaluators(z, vps, vss, mine_vps, mine_vss)
    outq.put((rank, r[0]["vpq"]["vpq_all"], float(r[0]["stq"]["STQ"]), float(r[1]["sem_seg"]["mIoU"]),
              float(r[1]["sem_seg"]["VC16"])))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world2_equals_world1(g11, tmp_path):
    import torch.multiprocessing as mp
    vps, vss = make_evaluators(g11, str(tmp_path / "w1"))
    gj, _, _ = _vipseg(g11)
    r1 = run_evaluators(g11, vps, vss, {v["video_id"] for v in gj["videos"]}, {str(v) for v in g11["vspw/videos"]})
    ref = (r1[0]["vpq"]["vpq_all"], float(r1[0]["stq"]["STQ"]), float(r1[1]["sem_seg"]["mIoU"]), float(r1[1]["sem_seg"]["VC16"]))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    init = "file://" + str(tmp_path / "pg_init")
    procs = [ctx.Process(target=_world2_worker, args=(r, str(tmp_path), init, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for _, *vals in got:
        assert tuple(vals) == ref


def _fake_detectron2(monkeypatch, entries):
    """detectron2.data.MetadataCatalog stand-in holding `entries` (name -> metadata namespace)."""
    import sys
    import types
    d2, data = types.ModuleType("detectron2"), types.ModuleType("detectron2.data")
    data.MetadataCatalog = types.SimpleNamespace(get=lambda name: entries[name])
    d2.data = data
    monkeypatch.setitem(sys.modules, "detectron2", d2)
    monkeypatch.setitem(sys.modules, "detectron2.data", data)


def test_evaluators_built_from_registered_metadata(g11, tmp_path, monkeypatch):
    """No keyword overrides: the ground truth and category maps come from metadata shaped like the reference's registrations
    (data_video/datasets/vps.py: panoptic_root / panoptic_json, identity thing / stuff id maps; vss.py: image_root =
    `<root>/VSPW_480p/data/`, ignore_label 255, stuff_dataset_id_to_contiguous_id {c: c}).  The same video processed twice
    (e.g. on two ranks) is accepted."""
    import types
    from dvis_plus_amd.evaluation import VPSEvaluator, VSSEvaluator
    root = str(tmp_path)
    truth, _, vspw, _ = rebuild_trees(g11, root)
    gj, pa, _ = _vipseg(g11)
    things = [c["id"] for c in gj["categories"] if c["isthing"]]
    stuff = [c["id"] for c in gj["categories"] if not c["isthing"]]
    image_root = os.path.join(root, "VSPW_480p", "data") + "/"
    os.rename(vspw, os.path.dirname(os.path.normpath(image_root)))
    _fake_detectron2(monkeypatch, {
        "panoVSPW_vps_video_val": types.SimpleNamespace(
            panoptic_root=truth, panoptic_json=os.path.join(root, "gt.json"),
            thing_dataset_id_to_contiguous_id={i: i for i in things}, stuff_dataset_id_to_contiguous_id={i: i for i in stuff}),
        "VSPW_vss_video_val": types.SimpleNamespace(
            image_root=image_root, ignore_label=255, stuff_dataset_id_to_contiguous_id={i: i for i in range(124)})})
    vps = VPSEvaluator("panoVSPW_vps_video_val", None, True, None, device="cpu")
    vss = VSSEvaluator("VSPW_vss_video_val", None, True, None, device="cpu")
    assert list(vss.video_order) == [str(v) for v in g11["vspw/videos"]]
    vps.reset()
    vss.reset()
    for v in gj["videos"]:
        inputs = [{"video_id": v["video_id"], "file_names": [f"img/{im['file_name'][:-4]}.jpg" for im in v["images"]],
                   "frame_idx": list(range(len(v["images"])))}]
        vps.process(inputs, vps_outputs(g11, v["video_id"], gj, pa))
    for vid in reversed(list(g11["vspw/videos"])):             # order restored from val.txt
        T = len(g11[f"vspw/{vid}/gt"])
        inputs = [{"video_id": str(vid), "file_names": [f"{image_root}{vid}/origin/{t:05d}.jpg" for t in range(T)],
                   "frame_idx": list(range(T))}]
        vss.process(inputs, {"pred_masks": torch.from_numpy(g11[f"vspw/{vid}/pred"].astype(np.int64)), "task": "vss"})
    r_vps, r_vss = vps.evaluate(), vss.evaluate()
    check_vipseg(g11, r_vps["vpq"], r_vps["stq"])
    check_vspw(g11, r_vss["sem_seg"], r_vss["sem_seg"])
    v0 = gj["videos"][0]
    inputs = [{"video_id": v0["video_id"], "file_names": [im["file_name"] for im in v0["images"]]}]
    vps.process(inputs, vps_outputs(g11, v0["video_id"], gj, pa))
    assert "vpq_all" in vps.evaluate()["vpq"]


def test_evaluators_without_metadata_or_overrides_raise(monkeypatch):
    import sys
    from dvis_plus_amd.evaluation import VSSEvaluator
    monkeypatch.setitem(sys.modules, "detectron2", None)         # `import detectron2.data` raises ImportError
    monkeypatch.setitem(sys.modules, "detectron2.data", None)
    with pytest.raises(RuntimeError, match="vspw_root"):
        VSSEvaluator("VSPW_vss_video_val", None, True, None)
