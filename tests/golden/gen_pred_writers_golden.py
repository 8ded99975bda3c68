"""Writes tests/golden/g13_pred_writers.npz: VIPSeg / VSPW prediction files written by the reference's own writers
(dvis_Plus/data_video/vps_eval.py, vss_eval.py) from small synthetic 24 x 40 clips.

    python tests/golden/gen_pred_writers_golden.py [/path/to/DVIS_Plus]      (default: _ref_import.REF)

Build-machine only, like gen_vis_golden.py; nothing at test time imports this file.  The two reference files are loaded
UNCHANGED by path, with stubs for the detectron2 names they import (comm, CfgNode, MetadataCatalog, DatasetEvaluator,
PathManager).  panopticapi is not installed, so `panopticapi.utils` is a stand-in: our own numpy rgb2id and IdGenerator below,
written from the package's documented colour rule (black and the stuff colours start out taken; stuff segments get the category
colour; a thing segment gets the category colour if free, else the colour plus np.random.randint(-30, 31, size=3) clipped to
[0, 255], redrawn until free).  np.random.seed(SEED + k) is set before video k.

Cases: two instances of one thing category (a jittered colour); two stuff segments of one category (same colour and id); a thing
category whose colour a stuff category already has; a colour near 255 (clipping); a segment empty on some frames; a listed
segment never present; a panoptic id that segments_infos does not list; a frame with no segment; frame names with two dots;
frame_idx a subset of file_names; VSS values >= 256 and < 0 (uint8 wrap), the ignore label, and a class with no mapping (KeyError).

Stored: the inputs (JSON + maps), every written PNG as bytes and decoded, and pred.json.
"""
import importlib.util
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _ref_import import REF, _mod as mod    # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "g13_pred_writers.npz")
H, W = 24, 40
SEED = 1300

# VIPSeg-like metadata: dataset ids, thing / stuff maps dataset id -> dataset id as datasets/vps.py registers them
CATEGORIES = [{"id": 2, "name": "person", "isthing": 1, "color": [220, 20, 60]},
              {"id": 4, "name": "car", "isthing": 1, "color": [250, 250, 5]},          # clipping at 255
              {"id": 7, "name": "dog", "isthing": 1, "color": [70, 130, 180]},          # = the colour of stuff 11
              {"id": 10, "name": "wall", "isthing": 0, "color": [120, 120, 120]},
              {"id": 11, "name": "sky", "isthing": 0, "color": [70, 130, 180]},
              {"id": 13, "name": "road", "isthing": 0, "color": [128, 64, 128]}]
THINGS = [c["id"] for c in CATEGORIES if c["isthing"]]
STUFF = [c["id"] for c in CATEGORIES if not c["isthing"]]
# VSPW-like: the id map is built from the keys; classes 0..5 are mapped, 6 is not
VSS_KEYS = [5, 6, 7, 8, 9, 20]
IGNORE = 255


# --- stand-in panopticapi.utils (numpy) ------------------------------------------------------------------------------------------
def rgb2id(color):
    if isinstance(color, np.ndarray) and color.ndim == 3:
        c = color.astype(np.int32)
        return c[..., 0] + 256 * c[..., 1] + 65536 * c[..., 2]
    return int(color[0] + 256 * color[1] + 65536 * color[2])


class IdGenerator:
    def __init__(self, categories):
        self.categories = categories
        self.used = {(0, 0, 0)} | {tuple(c["color"]) for c in categories.values() if c["isthing"] == 0}

    def get_color(self, cat_id):
        cat = self.categories[cat_id]
        if cat["isthing"] == 0:
            return cat["color"]
        if tuple(cat["color"]) not in self.used:
            self.used.add(tuple(cat["color"]))
            return cat["color"]
        while True:
            c = tuple(np.maximum(0, np.minimum(255, np.array(cat["color"]) + np.random.randint(-30, 31, size=3))))
            if c not in self.used:
                self.used.add(c)
                return c


# --- reference loading ------------------------------------------------------------------------------------------------------------
_META = {}


def load_reference(ref):
    class CfgNode(dict):
        pass

    class MetadataCatalog:
        @staticmethod
        def get(name):
            return _META[name]

    class PathManager:
        get_local_path = staticmethod(lambda p: p)
        mkdirs = staticmethod(lambda p: os.makedirs(p, exist_ok=True))

    comm = mod("detectron2.utils.comm", synchronize=lambda: None, gather=lambda x, dst=0: [x], is_main_process=lambda: True)
    mod("detectron2", utils=mod("detectron2.utils", comm=comm))
    mod("detectron2.config", CfgNode=CfgNode)
    mod("detectron2.data", MetadataCatalog=MetadataCatalog)
    mod("detectron2.evaluation", DatasetEvaluator=object)
    mod("detectron2.utils.file_io", PathManager=PathManager)
    mod("panopticapi", utils=mod("panopticapi.utils", rgb2id=rgb2id, IdGenerator=IdGenerator))
    out = []
    for name in ("vps_eval", "vss_eval"):
        spec = importlib.util.spec_from_file_location(f"ref_{name}", os.path.join(ref, "dvis_Plus", "data_video", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        out.append(m)
    return out


# --- synthetic clips ----------------------------------------------------------------------------------------------------------------
def vps_videos():
    """(video_id, file_names, frame_idx, pred_masks (T, H, W) int32, segments_infos)."""
    # v0: ids 1, 2 person (jitter), 3, 4 wall (two stuff segments of one category), 5 car (empty on frame 1), 6 dog (never present,
    # and its colour is sky's: jitter), 8 sky, 9 unlisted; frame 2 has no segment
    T = 4
    m = np.zeros((T, H, W), np.int32)
    for t in range(T):
        if t == 2:
            continue
        m[t, :, :W // 2] = 3
        m[t, :, W // 2:] = 4
        m[t, :6, :] = 8
        m[t, 5:12, 3 + t:10 + t] = 1
        m[t, 10:20, 22 - t:30 - t] = 2
        if t != 1:
            m[t, 14:22, 12:17] = 5
        m[t, 20:, 34:] = 9
    segs = [{"id": 1, "isthing": True, "category_id": 0}, {"id": 2, "isthing": True, "category_id": 0},
            {"id": 3, "isthing": False, "category_id": 3}, {"id": 4, "isthing": False, "category_id": 3},
            {"id": 5, "isthing": True, "category_id": 1}, {"id": 6, "isthing": True, "category_id": 2},
            {"id": 8, "isthing": False, "category_id": 4}]
    names0 = ["v0/00000.jpg", "v0/00001.a.jpg", "v0/00002.jpg", "v0/00003.b.c.jpg"]
    out = [("v0", names0, [0, 1, 2, 3], m, segs)]
    # v1: three cars (base, then two jittered near 255), a dog (base colour taken by sky: jitter), road; frame_idx a subset
    T = 3
    m = np.zeros((T, H, W), np.int32)
    for t in range(T):
        m[t] = 7
        m[t, 2:9, 2 + 2 * t:12 + 2 * t] = 2
        m[t, 12:20, 5:15] = 3
        m[t, 4:16, 25:33] = 5 if t != 0 else 7
        m[t, 18:23, 28:39] = 4
    segs = [{"id": 2, "isthing": True, "category_id": 1}, {"id": 3, "isthing": True, "category_id": 1},
            {"id": 4, "isthing": True, "category_id": 1}, {"id": 5, "isthing": True, "category_id": 2},
            {"id": 7, "isthing": False, "category_id": 5}]
    names1 = ["v1/%05d.f.jpg" % i for i in range(5)]
    out.append(("v1", names1, [1, 2, 4], m, segs))
    return out


def vss_videos():
    """(video_id, file_names, frame_idx, pred_masks (T, H, W) int64); the last one has an unmapped class."""
    T = 3
    m = np.zeros((T, H, W), np.int64)
    for t in range(T):
        m[t, :, :] = 1
        m[t, :, W // 2:] = 258                 # -> 2 after astype(uint8)
        m[t, 3:9, 4 + t:14 + t] = 255          # ignore label
        m[t, 12:20, 20:30] = 5 if t else -1    # -1 -> 255: ignore after the wrap
        m[t, 20:, :6] = 512 + 3                # -> 3
    ok = ("s0", ["s0/a.b.jpg", "s0/c.jpg", "s0/d.e.f.png"], [0, 1, 2], m)
    T = 2
    bad = np.ones((T, H, W), np.int64)
    bad[:, 4:8, 4:8] = 6 + 256                 # class 6: no mapping
    bad[:, 10:12, 10:12] = 7                   # class 7 too: the KeyError names the smaller
    return [ok, ("s1", ["s1/0.jpg", "s1/1.jpg"], [0, 1], bad)]


def main(ref):
    vps_eval, vss_eval = load_reference(ref)
    z = {}
    meta = {"categories": CATEGORIES, "things": THINGS, "stuff": STUFF, "vss_keys": VSS_KEYS, "ignore": IGNORE, "seed": SEED,
            "vps": [], "vss": []}
    with tempfile.TemporaryDirectory() as tmp:
        _META["g13_vps"] = types.SimpleNamespace(
            categories={c["id"]: c for c in CATEGORIES}, thing_dataset_id_to_contiguous_id={i: i for i in THINGS},
            stuff_dataset_id_to_contiguous_id={i: i for i in STUFF}, panoptic_json=os.path.join(tmp, "unused.json"))
        _META["g13_vss"] = types.SimpleNamespace(ignore_label=IGNORE, stuff_dataset_id_to_contiguous_id={k: i for i, k in
                                                                                                       enumerate(VSS_KEYS)})
        out_vps = os.path.join(tmp, "vps")
        ev = vps_eval.VPSEvaluator("g13_vps", None, False, out_vps)
        ev.reset()
        for k, (vid, names, fidx, m, segs) in enumerate(vps_videos()):
            np.random.seed(SEED + k)
            ev.process([{"video_id": vid, "file_names": names, "frame_idx": fidx}],
                       {"image_size": (H, W), "pred_masks": torch.from_numpy(m), "segments_infos": segs})
            meta["vps"].append({"video_id": vid, "file_names": names, "frame_idx": fidx, "segments_infos": segs})
            z[f"vps/{vid}/pred_masks"] = m
        ev.evaluate()
        z["vps/pred_json"] = np.frombuffer(open(os.path.join(out_vps, "pred.json"), "rb").read(), np.uint8)
        files = []
        for vid in sorted(os.listdir(os.path.join(out_vps, "pan_pred"))):
            for f in sorted(os.listdir(os.path.join(out_vps, "pan_pred", vid))):
                rel = f"pan_pred/{vid}/{f}"
                files.append(rel)
                data = open(os.path.join(out_vps, rel), "rb").read()
                z[f"vps/file/{rel}"] = np.frombuffer(data, np.uint8)
                z[f"vps/array/{rel}"] = np.array(Image.open(io.BytesIO(data)))
        meta["vps_files"] = files

        out_vss = os.path.join(tmp, "vss")
        ev = vss_eval.VSSEvaluator("g13_vss", None, False, out_vss)
        ev.reset()
        files = []
        for k, (vid, names, fidx, m) in enumerate(vss_videos()):
            inputs = [{"video_id": vid, "file_names": names, "frame_idx": fidx}]
            meta["vss"].append({"video_id": vid, "file_names": names, "frame_idx": fidx})
            z[f"vss/{vid}/pred_masks"] = m
            try:
                ev.process(inputs, {"image_size": (H, W), "pred_masks": torch.from_numpy(m)})
            except KeyError as e:
                meta["vss"][-1]["key_error"] = int(e.args[0])
                continue
            for f in sorted(os.listdir(os.path.join(out_vss, vid))):
                rel = f"{vid}/{f}"
                files.append(rel)
                data = open(os.path.join(out_vss, rel), "rb").read()
                z[f"vss/file/{rel}"] = np.frombuffer(data, np.uint8)
                z[f"vss/array/{rel}"] = np.array(Image.open(io.BytesIO(data)))
        meta["vss_files"] = files
        assert ev.evaluate() == {}
    z["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    np.savez_compressed(OUT, **z)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    print(bytes(z["vps/pred_json"]).decode()[:600])


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else REF)
