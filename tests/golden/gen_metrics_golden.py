"""Writes tests/golden/g11_video_metrics.npz: small synthetic VIPSeg / VSPW trees scored by the reference's own scripts.

    python tests/golden/gen_metrics_golden.py /path/to/DVIS_Plus

Build-machine only, like gen_golden.py; nothing at test time imports this file.  It synthesises the trees (PNGs, panoptic
JSON, val.txt) in a temporary directory, runs utils/eval_vpq_vspw.py, eval_stq_vspw.py, eval_miou_vspw.py and eval_vc_vspw.py
UNCHANGED as subprocesses (numpy >= 2 lacks `np.bool`, which segmentation_and_tracking_quality.py uses: the child aliases it to
`bool` before the script runs, when missing) and stores the input maps, the JSON and what the scripts print / write.

Cases covered: crowd GT segments; VOID on both sides; stuff merged into one predicted segment; unmatched and below-threshold
predictions; a GT id above 65535; a GT id in the PNG that the JSON does not list; a frame without any prediction; videos
shorter than 8 and 16 frames; VSPW labels 0 and 255; classes only in the GT or only in the prediction.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "g11_video_metrics.npz")
H, W = 24, 40
THINGS = set(range(58))          # VIPSeg: 58 thing classes, 66 stuff classes (ids 0..123)


def rgb(ids):
    ids = ids.astype(np.int64)
    return np.stack([ids % 256, ids // 256 % 256, ids // 65536], -1).astype(np.uint8)


def vipseg_video(rng, T, crowd, big_id, empty_frame):
    """One video: (gt ids (T,H,W), gt segments per frame, pred raw ids, pred segments per frame)."""
    gt = np.zeros((T, H, W), np.int64)
    pred = np.zeros((T, H, W), np.int64)
    gt_segs = [[] for _ in range(T)]
    pred_segs = [[] for _ in range(T)]
    stuff_a, stuff_b = 60 + rng.integers(0, 10), 80 + rng.integers(0, 10)
    # GT: two stuff regions, 3-4 moving thing boxes, a VOID strip, an unlisted id in a corner
    objs = [(int(rng.integers(0, 58)), int(rng.integers(2, 12)), int(rng.integers(2, 25)), int(rng.integers(5, 10)),
             int(rng.integers(6, 14))) for _ in range(4)]
    gid = {"sa": 1000 + int(stuff_a), "sb": big_id if big_id else 2000 + int(stuff_b)}
    for n in range(len(objs)):
        gid[n] = 300 + 7 * n + int(rng.integers(0, 5))
    fp_cat = 100 + int(rng.integers(0, 20))
    pid = {k: int(v) for k, v in zip(["sa", "sb", 0, 1, 2, 3, "fp"], rng.choice(np.arange(1, 1 << 24), 7, replace=False))}
    for t in range(T):
        g = np.zeros((H, W), np.int64)
        g[:, :W // 2] = gid["sa"]
        g[:, W // 2:] = gid["sb"]
        p = np.zeros((H, W), np.int64)
        p[:, :W // 2 + 2] = pid["sa"]
        p[:, W // 2 + 2:] = pid["sb"] if t % 3 else pid["sa"]           # stuff merged into one segment on some frames
        for n, (c, y, x, h, w) in enumerate(objs):
            yy, xx = y + (t % 4) // 2, (x + t) % (W - w)
            g[yy:yy + h, xx:xx + w] = gid[n]
            if n == 3:
                continue                                               # object 3: never predicted (FN)
            dy = 1 if n == 1 else 0
            pw = w if n != 2 else max(1, w // 3)                       # object 2: below the IoU threshold
            p[yy + dy:yy + dy + h, xx:xx + pw] = pid[n]
        g[H - 3:, :] = 0                                               # VOID strip
        g[0:2, 0:3] = 77                                               # in the PNG, not in the JSON
        p[0:3, W - 4:] = pid["fp"] if t % 2 else 0                     # an unmatched prediction / VOID prediction
        p[H - 2:, W - 6:] = pid["fp"] if t % 2 else 0                  # ... partly over VOID
        if empty_frame is not None and t == empty_frame:
            p[:] = 0
        gt[t], pred[t] = g, p
        cats = {gid["sa"]: int(stuff_a), gid["sb"]: int(stuff_b)}
        for n, (c, *_r) in enumerate(objs):
            cats[gid[n]] = c
        for i in np.unique(g):
            if i in cats:
                gt_segs[t].append({"id": int(i), "category_id": cats[int(i)], "area": int((g == i).sum()),
                                   "iscrowd": int(crowd and i == gid[0]), "bbox": [0, 0, 1, 1]})
        pcats = {pid["sa"]: int(stuff_a), pid["sb"]: int(stuff_b), pid["fp"]: fp_cat}
        for n, (c, *_r) in enumerate(objs):
            pcats[pid[n]] = c if n != 1 else (c + 1) % 58                  # object 1: the wrong class
        for i in np.unique(p):
            if i != 0:
                pred_segs[t].append({"id": int(i), "category_id": pcats[int(i)], "area": int((p == i).sum()), "iscrowd": 0})
    return gt, gt_segs, pred, pred_segs


def vspw_video(rng, T):
    gt = np.zeros((T, H, W), np.uint8)
    pred = np.zeros((T, H, W), np.uint8)
    a, b, c = (int(x) for x in rng.integers(1, 125, 3))
    for t in range(T):
        g = np.full((H, W), a, np.uint8)
        g[:, W // 2:] = b
        g[4:12, (3 + t // 3) % 20:(3 + t // 3) % 20 + 8] = c
        g[H - 2:, :] = 0                                                # label 0 -> 255 -> 254: dropped
        g[0, :5] = 255                                                  # label 255 -> 254: dropped
        p = np.full((H, W), a - 1, np.uint8)
        p[:, W // 2 + 1:] = b - 1
        p[4:12, (3 + t // 2) % 20:(3 + t // 2) % 20 + 8] = (c - 1) if t % 5 else 123   # 123: a class only predicted
        p[10:13, 30:33] = (t // 4) % 124
        gt[t], pred[t] = g, p
    return gt, pred


def run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{cmd} failed:\n{r.stdout}\n{r.stderr}")
    return r.stdout


CHILD = ("import sys, runpy, numpy as np\n"
         "if not hasattr(np, 'bool'): np.bool = bool\n"
         "script = sys.argv[1]; sys.argv = sys.argv[1:]; sys.path.insert(0, __import__('os').path.dirname(script))\n"
         "runpy.run_path(script, run_name='__main__')\n")


def main(ref_root):
    utils = os.path.join(ref_root, "utils")
    rng = np.random.default_rng(11)
    z = {}
    with tempfile.TemporaryDirectory() as tmp:
        # ---------------------------------------------------------------- VIPSeg-style tree
        truth, submit = os.path.join(tmp, "panomasksRGB"), os.path.join(tmp, "submit")
        cats = [{"id": i, "name": f"c{i}", "isthing": int(i in THINGS)} for i in range(124)]
        gt_json = {"categories": cats, "videos": [], "annotations": []}
        pred_json = {"annotations": []}
        specs = [("v0", 10, True, 0, None), ("v1", 3, False, 70001, None), ("v2", 9, True, 66000, 4)]
        for vid, T, crowd, big, empty in specs:
            gt, gsegs, pred, psegs = vipseg_video(rng, T, crowd, big, empty)
            names = [f"{t:05d}.png" for t in range(T)]
            os.makedirs(os.path.join(truth, vid))
            os.makedirs(os.path.join(submit, "pan_pred", vid))
            for t, n in enumerate(names):
                Image.fromarray(rgb(gt[t])).save(os.path.join(truth, vid, n))
                Image.fromarray(rgb(pred[t])).save(os.path.join(submit, "pan_pred", vid, n))
            gt_json["videos"].append({"video_id": vid, "images": [{"file_name": n} for n in names]})
            gt_json["annotations"].append({"video_id": vid, "annotations": [{"segments_info": s, "file_name": n}
                                                                             for s, n in zip(gsegs, names)]})
            pred_json["annotations"].append({"video_id": vid, "annotations": [{"segments_info": s, "file_name": n}
                                                                               for s, n in zip(psegs, names)]})
            z[f"vipseg/{vid}/gt"] = gt.astype(np.int32)
            z[f"vipseg/{vid}/pred"] = pred.astype(np.int32)
        gt_file = os.path.join(tmp, "panoptic_gt_val.json")
        with open(gt_file, "w") as f:
            json.dump(gt_json, f)
        with open(os.path.join(submit, "pred.json"), "w") as f:
            json.dump(pred_json, f)
        z["vipseg/gt_json"] = np.array(json.dumps(gt_json))
        z["vipseg/pred_json"] = np.array(json.dumps(pred_json))

        out = run([sys.executable, os.path.join(utils, "eval_vpq_vspw.py"), "--submit_dir", submit, "--truth_dir", truth,
                   "--pan_gt_json_file", gt_file, "--num_processes", "1"], tmp)
        triples = [ln.split() for ln in out.splitlines() if re.fullmatch(r"\S+ \S+ \S+", ln.strip())]
        vals = np.array([[float(x) for x in tr] for tr in triples if all(re.fullmatch(r"[-0-9.e]+", x) for x in tr)])
        assert vals.shape == (5, 3), out
        z["vipseg/out/vpq_per_nframes"] = vals                    # all / thing / stuff per nframes 1, 2, 4, 6, 8
        for nf in (1, 2, 4, 6, 8):
            txt = open(os.path.join(submit, "vpq-%d.txt" % ((nf - 1) * 5))).read()
            z[f"vipseg/out/vpq_txt_{nf}"] = np.array(txt)
            rows = [ln.split("|") for ln in txt.splitlines() if re.match(r"^\s*\d+ \|", ln)]
            table = np.array([[int(a)] + [float(x) for x in b.split()] for a, b in rows])
            z[f"vipseg/out/vpq_class_{nf}"] = table               # id, PQ, SQ, RQ, IoU, TP, FP, FN (as printed)
        z["vipseg/out/vpq_final_txt"] = np.array(open(os.path.join(submit, "vpq-final.txt")).read())

        code = os.path.join(tmp, "child.py")
        with open(code, "w") as f:
            f.write(CHILD)
        out = run([sys.executable, code, os.path.join(utils, "eval_stq_vspw.py"), "--submit_dir", submit, "--truth_dir",
                   truth, "--pan_gt_json_file", gt_file], tmp)
        stq = [float(re.search(r"^%s\s*:\s*(\S+)" % k, out, re.M).group(1)) for k in ("STQ", "AQ", "IoU")]
        z["vipseg/out/stq"] = np.array(stq)                      # STQ, AQ, IoU

        # ---------------------------------------------------------------- VSPW-style tree
        root, predd = os.path.join(tmp, "VSPW"), os.path.join(tmp, "vss_pred")
        vids = [("a0", 20), ("a1", 12), ("a2", 6), ("a3", 17)]
        with open(os.path.join(os.makedirs(root) or root, "val.txt"), "w") as f:
            f.write("".join(v + "\n" for v, _ in vids))
        for vid, T in vids:
            gt, pred = vspw_video(rng, T)
            os.makedirs(os.path.join(root, "data", vid, "mask"))
            os.makedirs(os.path.join(predd, vid))
            for t in range(T):
                Image.fromarray(gt[t]).save(os.path.join(root, "data", vid, "mask", f"{t:05d}.png"))
                Image.fromarray(pred[t]).save(os.path.join(predd, vid, f"{t:05d}.png"))
            z[f"vspw/{vid}/gt"], z[f"vspw/{vid}/pred"] = gt, pred
        z["vspw/videos"] = np.array([v for v, _ in vids])
        out = run([sys.executable, os.path.join(utils, "eval_miou_vspw.py"), root, predd], tmp)
        m = re.search(r"Acc:(\S+), Acc_class:(\S+), mIoU:(\S+), fwIoU: (\S+)", out)
        z["vspw/out/miou"] = np.array([float(x) for x in m.groups()])          # Acc, Acc_class, mIoU, fwIoU
        out = run([sys.executable, os.path.join(utils, "eval_vc_vspw.py"), root, predd], tmp)
        z["vspw/out/vc"] = np.array([float(re.search(r"VC%d score: (\S+)" % k, out).group(1)) for k in (8, 16)])
    np.savez_compressed(OUT, **z)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    for k in sorted(z):
        if "/out/" in k and z[k].dtype != object and z[k].dtype.kind == "f":
            print(k, z[k].tolist() if z[k].size < 8 else z[k].shape)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: gen_metrics_golden.py <DVIS_Plus checkout>")
    main(sys.argv[1])
