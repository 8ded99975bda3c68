"""VIS scoring on CPU tensors: the RLE codec, the host restatement of YTVOSeval and YTVISEvaluator reproduce the reference's
VIS evaluation exactly (fixture g12, written by tests/golden/gen_vis_golden.py from the unchanged reference files)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

from dvis_plus_amd import cpu_ops
from dvis_plus_amd import vis_metrics as VIS
from dvis_plus_amd.evaluation import YTVISEvaluator

CATS = [(3, "cat"), (7, "dog"), (11, "horse"), (20, "person")]
ID_MAP = {d: i for i, (d, _) in enumerate(CATS)}
NAMES = [n for _, n in CATS]


@pytest.fixture(scope="module")
def g12():
    return dict(np.load(os.path.join(GOLDEN, "g12_vis_metrics.npz")))


def text(z, key):
    return z[key].tobytes().decode()


def video_outputs(z, vid, device="cpu"):
    """The product's device task dict for fixture video `vid`: masks decoded from the stored runs."""
    P, T, H, W = (int(x) for x in z[f"v{vid}_shape"])
    runs, off = torch.from_numpy(z[f"v{vid}_runs"]), torch.from_numpy(z[f"v{vid}_run_off"])
    masks = cpu_ops.rle_decode(runs, off, H, W).bool().view(P, T, H, W) if P else torch.zeros((0, T, H, W), dtype=torch.bool)
    return ({"video_id": vid, "length": T},
            {"pred_scores": torch.from_numpy(z[f"v{vid}_scores"]).to(device),
             "pred_labels": torch.from_numpy(z[f"v{vid}_labels"]).to(device), "pred_masks": masks.to(device), "task": "vis"})


def make_evaluator(z, tmp, output_dir=True, gt=None, **kw):
    os.makedirs(tmp, exist_ok=True)
    path = os.path.join(tmp, "instances.json")
    with open(path, "w") as f:
        f.write(gt if gt is not None else text(z, "gt_json"))
    return YTVISEvaluator("ytvis_test", None, False, os.path.join(tmp, "out") if output_dir else None, json_file=path,
                          dataset_id_to_contiguous_id=ID_MAP, class_names=NAMES, **kw)


def run(z, ev, videos=None, device="cpu"):
    ev.reset()
    for vid in (videos if videos is not None else z["video_ids"]):
        inputs, outputs = video_outputs(z, int(vid), device)
        ev.process([inputs], outputs)
    return ev.evaluate()


def same_results(got, want):
    assert list(got) == list(want)
    for k, v in want.items():
        assert (math.isnan(v) and math.isnan(got[k])) or got[k] == v, (k, got[k], v)


# --- the string codec, pinned by hand ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("runs, want", [
    ([4], "4"),                 # 4 < 16: one group, no continuation: chr(48 + 4)
    ([0, 6, 1], "061"),         # pixel (0, 0) set: a leading empty run of zeros; i <= 2 take the counts as they are
    ([40], "X1"),               # 40 = 0b1_01000: group 8, x >> 5 = 1 -> more: 8 | 0x20 = 40 -> chr(88) 'X'; then 1 -> '1'
    ([5, 2, 1, 1], "521O"),     # i = 3: x = 1 - cnt[1] = -1: group 31 has 0x10 and x >> 5 = -1 -> done: chr(79) 'O'
    ([3, 17, 2, 17], "3a020"),  # 17: group 17 has 0x10 but x >> 5 = 0 != -1 -> more: 17 | 0x20 = 49 -> chr(97) 'a', then '0';
                                # i = 3: x = 17 - 17 = 0 -> '0'
    ([1, 2, 3, 40], "123V1"),   # i = 3 (strictly > 2): x = 40 - 2 = 38: group 6, x >> 5 = 1 -> 6 | 0x20 -> chr(86) 'V', '1'
])
def test_rle_strings_hand_derived(runs, want):
    r = torch.tensor(runs, dtype=torch.int32)
    chars, off = cpu_ops.rle_strings(r, torch.tensor([0, len(runs)]))
    got = bytes(chars.numpy()).decode()
    assert got == want
    assert VIS.rle_from_string(got).tolist() == runs


def test_rle_encode_decode_identity_on_random_masks():
    g = torch.Generator().manual_seed(3)
    for N, H, W in [(4, 7, 9), (3, 37, 53), (2, 1, 17), (2, 16, 1), (3, 64, 64)]:
        m = torch.rand((N, H, W), generator=g) < 0.4
        m[0] = True
        m[1, 0, 0] = True
        runs, off, area = cpu_ops.rle_encode(m)
        assert torch.equal(area, m.reshape(N, -1).sum(1))
        assert torch.equal(cpu_ops.rle_decode(runs, off, H, W).bool(), m)
        chars, soff = cpu_ops.rle_strings(runs, off)
        for n in range(N):
            s = bytes(chars[soff[n]:soff[n + 1]].numpy())
            assert VIS.rle_from_string(s).tolist() == runs[off[n]:off[n + 1]].tolist()
    assert cpu_ops.rle_encode(torch.ones((1, 3, 2), dtype=torch.bool))[0].tolist() == [0, 6]


# --- the reference's outputs ---------------------------------------------------------------------------------------------------------
def test_per_video_coco_json_matches_instances_to_coco_json_video(g12, tmp_path):
    ev = make_evaluator(g12, str(tmp_path))
    for vid in g12["video_ids"]:
        inputs, outputs = video_outputs(g12, int(vid))
        ev.reset()
        ev.process([inputs], outputs)
        preds = [d for v in ev._videos for d in v[0]]
        assert json.dumps(preds) == text(g12, f"v{vid}_coco_json"), vid


def test_evaluator_reproduces_the_reference(g12, tmp_path):
    ev = make_evaluator(g12, str(tmp_path))
    res = run(g12, ev)
    same_results(res["segm"], json.loads(text(g12, "results_dict"))["segm"])
    with open(tmp_path / "out" / "results.json") as f:
        assert f.read() == text(g12, "results_json")
    pth = torch.load(tmp_path / "out" / "instances_predictions.pth", weights_only=False)
    assert json.dumps(pth) == text(g12, "pth_json")


def test_host_scoring_tables_are_bit_equal(g12, tmp_path):
    """ious ==, precision / recall / scores array_equal, stats equal: the evaluator's own tables through vis_metrics.evaluate."""
    ev = make_evaluator(g12, str(tmp_path), output_dir=False)
    run(g12, ev)
    results = json.loads(text(g12, "results_json"))
    gt = VIS.YTVISGroundTruth(json.loads(text(g12, "gt_json")))
    dets, tables, n = [], {}, 0
    for preds, area, I, ga, frames in ev._videos:
        for p, r in enumerate(results[n:n + len(preds)]):
            dets.append(VIS.Detection(r["video_id"], r["category_id"], r["score"], area[p], n + p + 1))
        tables[preds[0]["video_id"]] = VIS.VideoTable(range(n, n + len(preds)), I, area[:, :frames].sum(1), ga)
        n += len(preds)
    e = VIS.evaluate(gt, dets, tables)
    keys = [tuple(k) for k in g12["iou_keys"]]
    assert keys == sorted(k for k, v in e["ious"].items() if len(v))
    for vid, cat in keys:
        got, want = e["ious"][vid, cat], g12[f"iou_{vid}_{cat}"]
        assert got.shape == want.shape and (got == want).all(), (vid, cat)
    for k in ("precision", "recall", "scores"):
        assert np.array_equal(e[k], g12[k]), k
    assert np.array_equal(e["stats"], g12["stats"])
    # the fixture covers what it claims: a NaN category, the medium / large ranges, > 100 detections of one class in a video
    assert np.isnan(VIS.derive_results(e, NAMES)["AP-horse"])
    assert (e["precision"][:, :, :, 2:, :] > -1).any(axis=(0, 1, 2, 4)).all()
    assert max(len(v) for v in e["ious"].values()) == 100


def test_command_line_scores_a_results_file(g12, tmp_path, capsys):
    gt = tmp_path / "instances.json"
    gt.write_text(text(g12, "gt_json"))
    res = tmp_path / "results.json"
    res.write_text(text(g12, "results_json"))
    got = VIS.main(["--gt", str(gt), "--results", str(res), "--device", "cpu"])
    same_results(got, json.loads(text(g12, "results_dict"))["segm"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1].replace("NaN", "null"))["segm"]["AP"] == got["AP"]


def test_without_annotations_only_results_json_is_written(g12, tmp_path):
    gj = json.loads(text(g12, "gt_json"))
    del gj["annotations"]
    ev = make_evaluator(g12, str(tmp_path), gt=json.dumps(gj))
    assert run(g12, ev) == {}
    with open(tmp_path / "out" / "results.json") as f:
        assert f.read() == text(g12, "results_json")


def _world2_worker(rank, root, init, outq):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=2)
    z = dict(np.load(os.path.join(GOLDEN, "g12_vis_metrics.npz")))
    ev = make_evaluator(z, os.path.join(root, f"r{rank}"))
    ev._distributed = True
    vids = list(z["video_ids"])
    half = (len(vids) + 1) // 2
    r = run(z, ev, vids[:half] if rank == 0 else vids[half:])
    outq.put((rank, json.dumps(r)))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world2_equals_world1(g12, tmp_path):
    import torch.multiprocessing as mp
    ref = run(g12, make_evaluator(g12, str(tmp_path / "w1")))
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
    for _, r in got:
        same_results(json.loads(r)["segm"], ref["segm"])
    with open(tmp_path / "r0" / "out" / "results.json") as f:
        assert f.read() == text(g12, "results_json")


def test_polygon_ground_truth_raises(g12, tmp_path):
    gj = json.loads(text(g12, "gt_json"))
    ann = gj["annotations"][0]
    ann["segmentations"][0] = [[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]]
    ev = make_evaluator(g12, str(tmp_path), gt=json.dumps(gj))
    inputs, outputs = video_outputs(g12, ann["video_id"])
    with pytest.raises(NotImplementedError, match=f"annotation {ann['id']}"):
        ev.process([inputs], outputs)


def test_size_mismatch_raises(g12, tmp_path):
    ev = make_evaluator(g12, str(tmp_path))
    inputs, outputs = video_outputs(g12, 1)
    outputs["pred_masks"] = outputs["pred_masks"][..., :-1]
    with pytest.raises(ValueError, match="video 1"):
        ev.process([inputs], outputs)


def test_reference_format_outputs_are_accepted(g12, tmp_path):
    """to_reference_format's form (python lists, per-instance CPU masks) gives the device form's results."""
    from dvis_plus_amd.postprocess import to_reference_format
    ev = make_evaluator(g12, str(tmp_path), output_dir=False)
    ev.reset()
    for vid in g12["video_ids"]:
        inputs, outputs = video_outputs(g12, int(vid))
        outputs["pred_ids"] = torch.arange(len(outputs["pred_scores"]))
        ev.process([inputs], to_reference_format(outputs))
    same_results(ev.evaluate()["segm"], json.loads(text(g12, "results_dict"))["segm"])
