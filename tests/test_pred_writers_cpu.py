"""CPU: the VIPSeg / VSPW prediction writers (dvis_plus_amd.pred_writers) against the files the reference's writers wrote (fixture
g13, tests/golden/gen_pred_writers_golden.py), and a round trip of fixture g11's predictions through the writers and the
video_metrics command line."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

from dvis_plus_amd import cpu_ops
from dvis_plus_amd import evaluation as E
from dvis_plus_amd import functions as Fn
from dvis_plus_amd import video_metrics as VM
from dvis_plus_amd.pred_writers import PanopticIdGenerator, rgb2id


@pytest.fixture(scope="module")
def g13():
    return dict(np.load(os.path.join(GOLDEN, "g13_pred_writers.npz")))


def meta(z):
    return json.loads(bytes(z["meta"]))


def vps_writer(z, out_dir, device="cpu", distributed=False):
    m = meta(z)
    return E.VPSPredictionWriter("g13_vps", None, distributed, out_dir, categories={c["id"]: c for c in m["categories"]},
                                 thing_dataset_id_to_contiguous_id={i: i for i in m["things"]},
                                 stuff_dataset_id_to_contiguous_id={i: i for i in m["stuff"]}, device=device)


def vss_writer(z, out_dir, device="cpu"):
    m = meta(z)
    return E.VSSPredictionWriter("g13_vss", None, False, out_dir,
                                 stuff_dataset_id_to_contiguous_id={k: i for i, k in enumerate(m["vss_keys"])},
                                 ignore_label=m["ignore"], device=device)


def vps_inputs(z, k, device="cpu"):
    v = meta(z)["vps"][k]
    pan = torch.from_numpy(z[f"vps/{v['video_id']}/pred_masks"]).to(device)
    return ([{"video_id": v["video_id"], "file_names": v["file_names"], "frame_idx": v["frame_idx"]}],
            {"image_size": tuple(pan.shape[1:]), "pred_masks": pan, "segments_infos": v["segments_infos"]})


def vss_inputs(z, k, device="cpu"):
    v = meta(z)["vss"][k]
    sem = torch.from_numpy(z[f"vss/{v['video_id']}/pred_masks"]).to(device)
    return [{"video_id": v["video_id"], "file_names": v["file_names"], "frame_idx": v["frame_idx"]}], {"pred_masks": sem}


def write_vps(z, out_dir, device="cpu", videos=None):
    w = vps_writer(z, out_dir, device)
    w.reset()
    for k in (videos if videos is not None else range(len(meta(z)["vps"]))):
        np.random.seed(meta(z)["seed"] + k)
        w.process(*vps_inputs(z, k, device))
    assert w.evaluate() == {}
    return w


def write_vss(z, out_dir, device="cpu"):
    w = vss_writer(z, out_dir, device)
    w.reset()
    for k, v in enumerate(meta(z)["vss"]):
        if "key_error" in v:
            continue
        w.process(*vss_inputs(z, k, device))
    assert w.evaluate() == {}
    return w


def listed(root):
    return sorted(os.path.relpath(os.path.join(d, f), root).replace(os.sep, "/") for d, _, fs in os.walk(root) for f in fs)


def check_vps_tree(z, root):
    from PIL import Image
    files = meta(z)["vps_files"]
    assert listed(root) == sorted(files + ["pred.json"])
    assert open(os.path.join(root, "pred.json"), "rb").read() == bytes(z["vps/pred_json"])
    for rel in files:
        assert np.array_equal(np.array(Image.open(os.path.join(root, rel))), z[f"vps/array/{rel}"]), rel
        assert open(os.path.join(root, rel), "rb").read() == bytes(z[f"vps/file/{rel}"]), rel


def check_vss_tree(z, root):
    from PIL import Image
    files = meta(z)["vss_files"]
    assert listed(root) == sorted(files)
    for rel in files:
        assert np.array_equal(np.array(Image.open(os.path.join(root, rel))), z[f"vss/array/{rel}"]), rel
        assert open(os.path.join(root, rel), "rb").read() == bytes(z[f"vss/file/{rel}"]), rel


def test_vps_files_equal_the_reference(g13, tmp_path):
    write_vps(g13, str(tmp_path))
    check_vps_tree(g13, str(tmp_path))


def test_vss_files_equal_the_reference(g13, tmp_path):
    write_vss(g13, str(tmp_path))
    check_vss_tree(g13, str(tmp_path))


def test_unmapped_vss_class_raises_key_error(g13, tmp_path):
    w = vss_writer(g13, str(tmp_path))
    w.reset()
    k = next(i for i, v in enumerate(meta(g13)["vss"]) if "key_error" in v)
    with pytest.raises(KeyError) as e:
        w.process(*vss_inputs(g13, k))
    assert e.value.args[0] == meta(g13)["vss"][k]["key_error"]
    assert not os.path.exists(os.path.join(str(tmp_path), meta(g13)["vss"][k]["video_id"]))
    assert w.evaluate() == {}


def test_colour_rule():
    cats = {1: {"isthing": 1, "color": [10, 250, 0]}, 2: {"isthing": 0, "color": [5, 5, 5]},
            3: {"isthing": 1, "color": [5, 5, 5]}}
    np.random.seed(0)
    g = PanopticIdGenerator(cats)
    assert g.get_color(2) == g.get_color(2) == (5, 5, 5)                  # stuff: the category colour, shared
    assert g.get_color(1) == (10, 250, 0)                                 # first thing: the base colour
    np.random.seed(0)
    want = tuple(int(x) for x in np.clip(np.array([10, 250, 0]) + np.random.randint(-30, 31, size=3), 0, 255))
    np.random.seed(0)
    assert g.get_color(1) == want and g.get_id(3) != rgb2id((5, 5, 5))   # later things jitter; a taken base colour too
    assert rgb2id((1, 2, 3)) == 1 + 2 * 256 + 3 * 65536


def test_kernel_formulations_on_small_maps():
    pan = torch.tensor([[[0, 1, 1], [2, 1, 7]], [[3, 3, 3], [3, 3, -1]]], dtype=torch.int32)
    stats, bad = Fn.pan_segment_stats(pan, 3)
    assert bad == 2
    assert stats[0].tolist() == [[1, 0, 0, 0, 0], [3, 1, 0, 2, 1], [1, 0, 1, 0, 1], [0, 0, 0, 0, 0]]
    assert stats[1, 3].tolist() == [5, 0, 0, 2, 1] and not stats[1, :3].any()
    rgb = Fn.pan_paint_rgb(pan, torch.tensor([0, 0x030201, 0xffffff], dtype=torch.int32))
    assert rgb.shape == (2, 2, 3, 3) and rgb[0, 0, 1].tolist() == [1, 2, 3] and rgb[0, 1, 0].tolist() == [255] * 3
    assert not rgb[1].any() and not rgb[0, 1, 2].any()
    lut = torch.full((256,), -1, dtype=torch.int32)
    lut[0], lut[255] = 7, 255
    out, bad = Fn.sem_paint(torch.tensor([0, 256, -1, 3, 259, 4]), lut)
    assert out.tolist() == [7, 7, 255, 255, 255, 255] and bad.nonzero().view(-1).tolist() == [3, 4] and bad[3] == 2


def _world2_worker(rank, root, init, q):
    import torch.distributed as dist
    try:
        dist.init_process_group("gloo", init_method=init, rank=rank, world_size=2)
        z = dict(np.load(os.path.join(GOLDEN, "g13_pred_writers.npz")))
        w = vps_writer(z, os.path.join(root, "w2"), distributed=True)
        w.reset()
        k = rank                                                  # rank r writes video r
        np.random.seed(meta(z)["seed"] + k)
        w.process(*vps_inputs(z, k))
        res = w.evaluate()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, res))
    except Exception as e:                                        # report, do not hang the parent
        q.put((rank, repr(e)))


def test_gloo_world2_writes_the_same_files(g13, tmp_path):
    import torch.multiprocessing as mp
    assert len(meta(g13)["vps"]) == 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    init = "file://" + str(tmp_path / "pg_init")
    procs = [ctx.Process(target=_world2_worker, args=(r, str(tmp_path), init, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(60)
    assert got == {0: {}, 1: {}}, got
    check_vps_tree(g13, str(tmp_path / "w2"))


# --- round trip of g11 through the writers and the video_metrics command line ---------------------------------------------------
VIPSEG_THINGS = 58


def g11_vps_outputs(z11, vid, pred_js):
    """g11's raw predicted ids and pred.json -> the product's output form: dense ids 1..n, segments_infos with contiguous
    categories (VIPSeg's maps are the identity on dataset ids, so contiguous = dataset id)."""
    raw = z11[f"vipseg/{vid}/pred"]
    cat = {}
    for frame in pred_js:
        for s in frame["segments_info"]:
            assert cat.setdefault(s["id"], s["category_id"]) == s["category_id"]
    table = sorted(cat)
    dense = VM.map_pred_ids(torch.from_numpy(raw), table, True)
    segs = [{"id": d + 1, "isthing": cat[r] < VIPSEG_THINGS, "category_id": cat[r]} for d, r in enumerate(table)]
    return dense, segs


def vipseg_categories():
    """124 VIPSeg-like categories with distinct colours (g11's GT JSON carries none)."""
    return {i: {"id": i, "isthing": int(i < VIPSEG_THINGS), "color": [i, 100, 200]} for i in range(124)}


def roundtrip(z11, root, device):
    import test_video_metrics_cpu as M
    truth, _, vspw, _ = M.rebuild_trees(z11, root)
    gj, pa, _ = M._vipseg(z11)
    submit = os.path.join(root, "written_vps")
    w = E.VPSPredictionWriter("g11", None, False, submit, categories=vipseg_categories(),
                              thing_dataset_id_to_contiguous_id={i: i for i in range(VIPSEG_THINGS)},
                              stuff_dataset_id_to_contiguous_id={i: i for i in range(VIPSEG_THINGS, 124)}, device=device)
    w.reset()
    for k, v in enumerate(gj["videos"]):
        vid = v["video_id"]
        dense, segs = g11_vps_outputs(z11, vid, pa[vid])
        stuff_cats = [s["category_id"] for s in segs if not s["isthing"]]
        # Two predicted stuff segments of one category would share a colour and an id in the written files (the reference's
        # merge); the VPQ / STQ to compare with would then be VPSEvaluator's on the merged map.  g11 has no such video.
        assert len(stuff_cats) == len(set(stuff_cats)), vid
        names = [f"{vid}/{os.path.splitext(im['file_name'])[0]}.jpg" for im in v["images"]]
        np.random.seed(k)
        w.process([{"video_id": vid, "file_names": names, "frame_idx": list(range(len(names)))}],
                  {"image_size": tuple(dense.shape[1:]), "pred_masks": dense.to(device), "segments_infos": segs})
    w.evaluate()
    vss_out = os.path.join(root, "written_vss")
    w = E.VSSPredictionWriter("g11", None, False, vss_out, stuff_dataset_id_to_contiguous_id={i: i for i in range(255)},
                              ignore_label=255, device=device)
    w.reset()
    for vid in z11["vspw/videos"]:
        vid = str(vid)
        pred = torch.from_numpy(z11[f"vspw/{vid}/pred"].astype(np.int32))
        names = [f"{vid}/{t:05d}.jpg" for t in range(len(pred))]
        w.process([{"video_id": vid, "file_names": names, "frame_idx": list(range(len(names)))}], {"pred_masks": pred.to(device)})
    w.evaluate()
    common = ["--submit_dir", submit, "--truth_dir", truth, "--pan_gt_json_file", os.path.join(root, "gt.json"),
              "--device", device]
    M.check_vipseg(z11, VM.main(["vpq", *common]), VM.main(["stq", *common]))
    M.check_vspw(z11, VM.main(["miou", vspw, vss_out, "--device", device]), VM.main(["vc", vspw, vss_out, "--device", device]))


def test_written_trees_score_like_the_reference(tmp_path, capsys):
    roundtrip(np.load(os.path.join(GOLDEN, "g11_video_metrics.npz")), str(tmp_path), "cpu")


def test_cpu_formulation_matches_a_direct_loop():
    g = torch.Generator().manual_seed(5)
    pan = torch.randint(-2, 9, (3, 7, 11), generator=g, dtype=torch.int32)
    stats, bad = cpu_ops.pan_segment_stats(pan, 6)
    assert bad == int(((pan < 0) | (pan > 6)).sum())
    for t in range(3):
        for i in range(7):
            ys, xs = np.nonzero(pan[t].numpy() == i)
            want = [len(ys), xs.min(), ys.min(), xs.max(), ys.max()] if len(ys) else [0] * 5
            assert stats[t, i].tolist() == [int(v) for v in want]
