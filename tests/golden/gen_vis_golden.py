"""Writes tests/golden/g12_vis_metrics.npz: a small synthetic YouTube-VIS dataset and predictions, scored by the reference's own
VIS evaluation (dvis_Plus/data_video/ytvis_eval.py, datasets/ytvis_api/ytvos.py, ytvoseval.py).

    python tests/golden/gen_vis_golden.py [/path/to/DVIS_Plus]      (default: _ref_import.REF)

Build-machine only, like gen_metrics_golden.py; nothing at test time imports this file.  The three reference files are loaded
UNCHANGED by path, under stand-in parent packages (dvis_Plus/data_video/__init__.py would pull in the dataset mappers), with
stubs for the detectron2 names they import (comm, CfgNode, MetadataCatalog, DatasetEvaluator, PathManager, create_small_table).
pycocotools is not installed, so `pycocotools.mask` is a stand-in: our own numpy code below (encode, decode, area, toBbox, merge,
frPyObjects for uncompressed RLE), written from the public description of COCO's RLE.  numpy >= 1.24 lacks `np.float`, which
ytvoseval.py's accumulate uses: it is aliased to `float` before the files load.

Cases: GT frames without a segmentation and a GT track absent in every frame (avg_area 0); a crowd GT; a GT whose JSON areas
differ from its mask areas; compressed and uncompressed GT counts; predictions with empty frames and a fully empty track; equal
scores inside one (video, category); 105 detections of one category in one video; a category without GT (per-category NaN); a
video without predictions; pixel (0, 0) set, full-column runs across the column wrap, an all-ones frame; W not a multiple of 4
or 64 and H * W not a multiple of 64; videos of 272 x 480 and 288 x 512 with small, medium and large tracks.
"""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _ref_import import REF, _mod as mod    # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "g12_vis_metrics.npz")
CATS = [(3, "cat"), (7, "dog"), (11, "horse"), (20, "person")]     # dataset ids, not contiguous; "horse" has no GT


# --- stand-in pycocotools.mask (numpy) --------------------------------------------------------------------------------------------
def _runs(m):
    """COCO runs of one (H, W) mask: column-major, zeros first."""
    v = np.asarray(m, dtype=np.uint8).reshape(m.shape[0], m.shape[1]).T.reshape(-1) != 0
    runs, cur, n = [], False, 0
    for x in v:
        if x != cur:
            runs.append(n)
            cur, n = x, 0
        n += 1
    runs.append(n)
    return runs


def _to_string(cnts):
    out = []
    for i, c in enumerate(cnts):
        x = int(c) - (int(cnts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5
            more = (x != -1) if ch & 0x10 else (x != 0)
            if more:
                ch |= 0x20
            out.append(chr(ch + 48))
    return "".join(out).encode()


def _from_string(s):
    if isinstance(s, str):
        s = s.encode()
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = c & 0x20
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x & 0xffffffff)
    return cnts


def _cnts(rle):
    c = rle["counts"]
    return list(c) if isinstance(c, list) else _from_string(c)


def _decode1(rle):
    h, w = rle["size"]
    v = np.zeros(h * w, np.uint8)
    pos = 0
    for i, c in enumerate(_cnts(rle)):
        if i & 1:
            v[pos:pos + c] = 1
        pos += c
    return v.reshape(w, h).T


def _encode1(m):
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": _to_string(_runs(m))}


def encode(a):
    a = np.asarray(a)
    if a.ndim == 2:
        return _encode1(a)
    return [_encode1(a[:, :, i]) for i in range(a.shape[2])]


def decode(r):
    if isinstance(r, list):
        return np.stack([_decode1(x) for x in r], 2)
    return _decode1(r)


def area(r):
    if isinstance(r, list):
        return np.array([area(x) for x in r], np.uint32)
    return np.uint32(sum(c for i, c in enumerate(_cnts(r)) if i & 1))


def toBbox(r):
    if isinstance(r, list):
        return np.stack([toBbox(x) for x in r])
    m = _decode1(r)
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return np.zeros(4)
    return np.array([xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1], np.float64)


def merge(rles, intersect=False):
    ms = [_decode1(r) for r in rles]
    out = ms[0].copy()
    for m in ms[1:]:
        out = (out & m) if intersect else (out | m)
    return _encode1(out)


def frPyObjects(obj, h, w):
    if isinstance(obj, list):
        if obj and isinstance(obj[0], dict):
            return [frPyObjects(o, h, w) for o in obj]
        raise NotImplementedError("polygons are not part of this stand-in")
    if isinstance(obj.get("counts"), list):
        return {"size": [h, w], "counts": _to_string(obj["counts"])}
    return obj


# --- reference loading ------------------------------------------------------------------------------------------------------------
class _Meta(types.SimpleNamespace):
    def get(self, k, default=None):
        return getattr(self, k, default)


_META = {}


def load_reference(ref):
    if not hasattr(np, "float"):
        np.float = float
    mk = types.ModuleType("pycocotools.mask")
    for k in ("encode", "decode", "area", "toBbox", "merge", "frPyObjects"):
        setattr(mk, k, globals()[k])
    pc = types.ModuleType("pycocotools")
    pc.mask = mk
    sys.modules.update({"pycocotools": pc, "pycocotools.mask": mk})

    class CfgNode(dict):
        pass

    class MetadataCatalog:
        @staticmethod
        def get(name):
            return _META[name]

    class PathManager:
        get_local_path = staticmethod(lambda p: p)
        open = staticmethod(open)
        mkdirs = staticmethod(lambda p: os.makedirs(p, exist_ok=True))

    comm = mod("detectron2.utils.comm", synchronize=lambda: None, gather=lambda x, dst=0: [x], is_main_process=lambda: True)
    mod("detectron2", utils=mod("detectron2.utils", comm=comm))
    mod("detectron2.config", CfgNode=CfgNode)
    mod("detectron2.data", MetadataCatalog=MetadataCatalog)
    mod("detectron2.evaluation", DatasetEvaluator=object)
    mod("detectron2.utils.file_io", PathManager=PathManager)
    mod("detectron2.utils.logger", create_small_table=lambda d: str(d))
    for name, path in (("dvis_Plus", "dvis_Plus"), ("dvis_Plus.data_video", "dvis_Plus/data_video"),
                       ("dvis_Plus.data_video.datasets", "dvis_Plus/data_video/datasets"),
                       ("dvis_Plus.data_video.datasets.ytvis_api", "dvis_Plus/data_video/datasets/ytvis_api")):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(ref, path)]
        sys.modules[name] = m
    return importlib.import_module("dvis_Plus.data_video.ytvis_eval")


# --- synthetic dataset ------------------------------------------------------------------------------------------------------------
def box(H, W, y, x, h, w):
    m = np.zeros((H, W), bool)
    m[max(0, y):max(0, y + h), max(0, x):max(0, x + w)] = True
    return m


def make_video(rng, vid, H, W, T, objs):
    """objs: list of (category dataset id, size (h, w), flags) -> (GT masks (G, T, H, W), GT annotation entries)."""
    gts, anns = [], []
    for j, (cat, (h, w), flags) in enumerate(objs):
        y0, x0 = int(rng.integers(0, max(1, H - h))), int(rng.integers(0, max(1, W - w)))
        m = np.stack([box(H, W, y0 + t, x0 + 2 * t, h, w) for t in range(T)])
        present = np.ones(T, bool)
        if "gaps" in flags:
            present[1::3] = False
        if "absent" in flags:
            present[:] = False
        m[~present] = False
        gts.append(m)
        anns.append({"cat": cat, "present": present, "crowd": "crowd" in flags, "skew_area": "skew" in flags,
                     "uncompressed": "raw" in flags})
    return np.stack(gts) if gts else np.zeros((0, T, H, W), bool), anns


def perturb(rng, m, shift):
    dy, dx = int(rng.integers(-shift, shift + 1)), int(rng.integers(-shift, shift + 1))
    return np.roll(np.roll(m, dy, -2), dx, -1)


def build():
    rng = np.random.default_rng(12)
    cid = {d: i for i, (d, _) in enumerate(CATS)}
    specs = [
        # id, H, W, T, objects, predictions (kind)
        (1, 24, 40, 4, [(3, (6, 8), ""), (3, (5, 5), "gaps"), (7, (7, 9), "crowd"), (20, (4, 4), "absent")], "mixed"),
        (2, 37, 53, 5, [(20, (10, 12), "raw"), (7, (8, 20), "skew")], "edge"),
        (3, 272, 480, 3, [(3, (200, 340), ""), (7, (150, 150), "raw"), (20, (60, 80), "gaps")], "mixed"),
        (4, 288, 512, 3, [(20, (260, 300), ""), (3, (100, 200), ""), (7, (20, 20), "")], "mixed"),
        (5, 24, 40, 3, [(3, (6, 6), ""), (7, (5, 9), "")], "many"),
        (6, 24, 40, 3, [(20, (8, 8), "")], "none"),
        (7, 33, 65, 4, [(7, (12, 30), "")], "ties"),
    ]
    videos, annotations, preds = [], [], []
    ann_id = 1
    for vid, H, W, T, objs, kind in specs:
        gm, anns = make_video(rng, vid, H, W, T, objs)
        videos.append({"id": vid, "height": H, "width": W, "length": T,
                       "file_names": [f"v{vid}/{t:05d}.jpg" for t in range(T)]})
        for j, a in enumerate(anns):
            segs, areas = [], []
            for t in range(T):
                if not a["present"][t]:
                    segs.append(None)
                    areas.append(None)
                    continue
                r = _encode1(gm[j, t])
                segs.append({"size": [H, W], "counts": _runs(gm[j, t]) if a["uncompressed"] else r["counts"].decode()})
                ar = int(gm[j, t].sum())
                areas.append(ar * 3 + 1 if a["skew_area"] else ar)
            annotations.append({"id": ann_id, "video_id": vid, "category_id": a["cat"], "iscrowd": int(a["crowd"]),
                                "segmentations": segs, "areas": areas, "bboxes": [None] * T, "height": H, "width": W,
                                "length": T})
            ann_id += 1
        # predictions (contiguous labels, float32 scores)
        pm, sc, lb = [], [], []
        if kind in ("mixed", "edge", "ties"):
            for j, a in enumerate(anns):
                pm.append(perturb(rng, gm[j], 2))
                sc.append(rng.random())
                lb.append(cid[a["cat"]])
                pm.append(perturb(rng, gm[j], 6))                          # a weaker duplicate
                sc.append(rng.random() * 0.5)
                lb.append(cid[a["cat"]] if j % 2 else cid[11])
            fp = np.zeros((T, H, W), bool)
            fp[:, :H // 3, :W // 3] = True
            fp[1] = False                                                   # an empty frame
            pm.append(fp)
            sc.append(0.3)
            lb.append(cid[20])
            pm.append(np.zeros((T, H, W), bool))                            # a fully empty track
            sc.append(0.05)
            lb.append(cid[3])
        if kind == "edge":
            e = np.zeros((T, H, W), bool)
            e[0, 0, 0] = True                                               # pixel (0, 0)
            e[1, :, 3:7] = True                                             # full columns: runs across the column wrap
            e[2] = True                                                     # an all-ones frame
            e[3, H - 1, :] = True
            e[4, :, W - 1] = True
            pm.append(e)
            sc.append(0.6)
            lb.append(cid[7])
        if kind == "ties":
            for _ in range(3):
                pm.append(perturb(rng, gm[0], 3))
                sc.append(0.5)                                              # equal scores: mergesort order decides
                lb.append(cid[7])
        if kind == "many":
            for k in range(105):
                pm.append(perturb(rng, gm[k % 2], 4))
                sc.append(float(rng.integers(0, 20)) / 20)
                lb.append(cid[3])
        preds.append((vid, T, np.stack(pm) if pm else np.zeros((0, T, H, W), bool),
                      np.asarray(sc, np.float32), np.asarray(lb, np.int64)))
    dataset = {"info": {}, "licenses": [], "videos": videos,
               "categories": [{"id": d, "name": n, "supercategory": "x"} for d, n in CATS], "annotations": annotations}
    return dataset, preds


def main(ref):
    mod = load_reference(ref)
    dataset, preds = build()
    cap = {}
    orig = mod._evaluate_predictions_on_coco

    def observed(*a, **k):
        cap["eval"] = orig(*a, **k)
        return cap["eval"]
    mod._evaluate_predictions_on_coco = observed
    with tempfile.TemporaryDirectory() as tmp:
        gt_path = os.path.join(tmp, "instances.json")
        with open(gt_path, "w") as f:
            json.dump(dataset, f)
        _META["synthetic_ytvis"] = _Meta(json_file=gt_path,
                                         thing_dataset_id_to_contiguous_id={d: i for i, (d, _) in enumerate(CATS)},
                                         thing_classes=[n for _, n in CATS])
        out_dir = os.path.join(tmp, "out")
        with contextlib.redirect_stdout(io.StringIO()):
            ev = mod.YTVISEvaluator("synthetic_ytvis", None, False, out_dir)
            ev.reset()
            per_video = []
            for vid, T, pm, sc, lb in preds:
                inputs = [{"video_id": vid, "length": T}]
                outputs = {"pred_scores": torch.from_numpy(sc).tolist(), "pred_labels": lb.tolist(),
                           "pred_masks": [torch.from_numpy(m) for m in pm]}
                per_video.append(json.dumps(mod.instances_to_coco_json_video(inputs, outputs)))
                ev.process(inputs, outputs)
            results = ev.evaluate()
        with open(os.path.join(out_dir, "results.json")) as f:
            results_json = f.read()
        pth = torch.load(os.path.join(out_dir, "instances_predictions.pth"), weights_only=False)
    e = cap["eval"]
    arrays = {"gt_json": np.frombuffer(json.dumps(dataset).encode(), np.uint8),
              "results_json": np.frombuffer(results_json.encode(), np.uint8),
              "pth_json": np.frombuffer(json.dumps(pth).encode(), np.uint8),
              "results_dict": np.frombuffer(json.dumps(results).encode(), np.uint8),
              "precision": e.eval["precision"], "recall": e.eval["recall"], "scores": e.eval["scores"],
              "stats": np.asarray(e.stats), "video_ids": np.array([p[0] for p in preds])}
    iou_keys = []
    for (vid, cat), iou in sorted(e.ious.items()):
        if len(iou) == 0:
            continue
        arrays[f"iou_{vid}_{cat}"] = np.asarray(iou)
        iou_keys.append((vid, cat))
    arrays["iou_keys"] = np.array(iou_keys, np.int64)
    for n, (vid, T, pm, sc, lb) in enumerate(preds):
        P, _, H, W = pm.shape
        runs = [_runs(pm[p, t]) for p in range(P) for t in range(T)]
        arrays[f"v{vid}_runs"] = np.concatenate([np.asarray(r, np.int32) for r in runs]) if runs else np.zeros(0, np.int32)
        arrays[f"v{vid}_run_off"] = np.concatenate(([0], np.cumsum([len(r) for r in runs]))).astype(np.int64)
        arrays[f"v{vid}_shape"] = np.array([P, T, H, W], np.int64)
        arrays[f"v{vid}_scores"] = sc
        arrays[f"v{vid}_labels"] = lb
        arrays[f"v{vid}_coco_json"] = np.frombuffer(per_video[n].encode(), np.uint8)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): {json.dumps(results)}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else REF)
