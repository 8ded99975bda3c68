"""VPS / VSS video metrics: VPQ, STQ, mIoU and VC from integer histograms computed on the device.

The reference scores VIPSeg / VSPW with four offline scripts (DVIS_Plus/utils/eval_vpq_vspw.py, eval_stq_vspw.py +
segmentation_and_tracking_quality.py, eval_miou_vspw.py, eval_vc_vspw.py) that decode every PNG again and run np.unique /
full-frame compares once per window and segment.  Here the pixels are read once per clip by the kernels of
csrc/video_metrics.hip (functions.pan_pair_hist / sem_confusion / video_consistency; CPU tensors take the bincount formulation of
cpu_ops.py) and everything else is host arithmetic on the small count tables, in float64 and in the reference's order:

  VPQ               per-frame (GT segment, predicted segment) counts -> prefix sums over frames -> the tube statistics of
                    every window start and length (eval_vpq_vspw.py:77-216) without another pass over the pixels
  STQ               the same per-frame counts -> per-sequence class confusion and track pair areas
                    (segmentation_and_tracking_quality.py:131-275, STQuality(124, things, 255, 16, 2**24))
  SemSegConfusion   the VSPW class confusion -> Acc / Acc_class / mIoU / fwIoU (eval_miou_vspw.py: Evaluator)
  VideoConsistency  per-window constant-pixel counts -> VC_k (eval_vc_vspw.py)

Command line (the reference scripts' arguments and directory layouts; prediction directories are rescored as they are):

  python -m dvis_plus_amd.video_metrics vpq --submit_dir DIR --truth_dir GT_DIR --pan_gt_json_file GT.json
  python -m dvis_plus_amd.video_metrics stq --submit_dir DIR --truth_dir GT_DIR --pan_gt_json_file GT.json
  python -m dvis_plus_amd.video_metrics miou VSPW_DIR PRED_DIR
  python -m dvis_plus_amd.video_metrics vc VSPW_DIR PRED_DIR

Assumption shared with the reference's data: a segment id keeps its category (and crowd flag) within a video.
"""
import argparse
import collections
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import functions as Fn

VPQ_NFRAMES = (1, 2, 4, 6, 8)
OFFSET = 256 * 256 * 256
STQ_ARGS = dict(num_classes=124, ignore_label=255, label_bit_shift=16, offset=2 ** 24)
_EPSILON = 1e-15
MAX_DECODE_THREADS = 16


# ----------------------------------------------------------------------------------------------------------------------------
# per-video segment tables
# ----------------------------------------------------------------------------------------------------------------------------
class PanopticGT:
    """The GT segments of one video from its per-frame JSON annotations (``[{"segments_info": [{id, category_id, iscrowd,
    area}, ...]}, ...]``): ids sorted (the kernel's table), and per frame which are listed, their JSON area and position."""

    def __init__(self, frame_annotations):
        T = len(frame_annotations)
        first = collections.OrderedDict()           # id -> segment info of its first listing (video order)
        for ann in frame_annotations:
            for el in ann["segments_info"]:
                first.setdefault(int(el["id"]), el)
        if 0 in first:
            raise ValueError("GT segment id 0 is VOID and cannot be listed")
        self.table = np.array(sorted(first), dtype=np.int64)
        ng = len(self.table)
        row = {int(i): r for r, i in enumerate(self.table)}
        self.category = np.array([int(first[int(i)]["category_id"]) for i in self.table], dtype=np.int64)
        self.iscrowd = np.array([int(first[int(i)].get("iscrowd", 0)) for i in self.table], dtype=np.int64)
        self.inst = np.zeros(ng, dtype=np.int64)        # STQ instance number: order of first appearance in the JSON
        for n, i in enumerate(first):
            self.inst[row[i]] = n
        self.area = np.zeros((T, ng), dtype=np.int64)
        self.listed = np.zeros((T, ng), dtype=bool)
        self.pos = np.full((T, ng), -1, dtype=np.int64)  # position of the first listing of the id in the frame's JSON
        for t, ann in enumerate(frame_annotations):
            for n, el in enumerate(ann["segments_info"]):
                r = row[int(el["id"])]
                self.area[t, r] += int(el.get("area", 0))
                if not self.listed[t, r]:
                    self.pos[t, r] = n
                self.listed[t, r] = True

    @property
    def num_frames(self):
        return self.area.shape[0]


class PanopticPred:
    """The predicted segments of one video: dense ids 1..Np (0 = VOID) with their categories.  `listed` (T, Np + 1): the
    frames whose JSON lists the segment (None: the frames where it is present, as the reference's VPSEvaluator writes it);
    `inst` (Np + 1): STQ instance numbers (None: order of first appearance, frames in order, ids ascending)."""

    def __init__(self, category, listed=None, inst=None):
        self.category = np.asarray(category, dtype=np.int64)
        self.listed = None if listed is None else np.asarray(listed, dtype=bool)
        self.inst = None if inst is None else np.asarray(inst, dtype=np.int64)

    @property
    def num_pred(self):
        return len(self.category) - 1

    @classmethod
    def from_json(cls, frame_annotations):
        """Prediction JSON of the reference format: raw ids (r + 256 g + 65536 b).  Returns (PanopticPred, sorted raw ids):
        dense id d stands for raw id table[d - 1]."""
        first = collections.OrderedDict()
        for ann in frame_annotations:
            for el in ann["segments_info"]:
                first.setdefault(int(el["id"]), el)
        if 0 in first:
            raise ValueError("predicted segment id 0 is VOID and cannot be listed")
        table = np.array(sorted(first), dtype=np.int64)
        dense = {int(i): d + 1 for d, i in enumerate(table)}
        cat = np.full(len(table) + 1, -1, dtype=np.int64)
        inst = np.full(len(table) + 1, 255, dtype=np.int64)
        for n, i in enumerate(first):
            cat[dense[i]] = int(first[i]["category_id"])
            inst[dense[i]] = n
        listed = np.zeros((len(frame_annotations), len(table) + 1), dtype=bool)
        for t, ann in enumerate(frame_annotations):
            for el in ann["segments_info"]:
                listed[t, dense[int(el["id"])]] = True
        return cls(cat, listed, inst), table

    def resolve(self, present):
        """(listed, inst) given the per-frame presence (T, Np + 1) from the pair histogram."""
        listed = (present if self.listed is None else self.listed).copy()
        listed[:, 0] = False
        if self.inst is not None:
            return listed, self.inst
        inst = np.full(self.num_pred + 1, 255, dtype=np.int64)
        n = 0
        for t in range(listed.shape[0]):
            for d in np.nonzero(listed[t])[0]:
                if inst[d] == 255:
                    inst[d] = n
                    n += 1
        return listed, inst


def pair_hist(gt_map, pred_map, gt: PanopticGT, num_pred):
    """(T, Ng + 2, Np + 1) int64 numpy counts of a clip (the kernel on GPU tensors, bincount on CPU tensors)."""
    table = torch.as_tensor(gt.table, dtype=torch.int32, device=gt_map.device)
    return Fn.pan_pair_hist(gt_map, pred_map, table, num_pred).cpu().numpy()


def _window_any(flags, nf):
    """flags (T, n) bool -> (T - nf + 1, n): any over frames [i, i + nf)."""
    c = np.concatenate([np.zeros((1, flags.shape[1]), np.int64), np.cumsum(flags, 0, dtype=np.int64)])
    return (c[nf:] - c[:-nf]) > 0


# ----------------------------------------------------------------------------------------------------------------------------
# VPQ
# ----------------------------------------------------------------------------------------------------------------------------
def _new_pq_stat():
    return collections.defaultdict(lambda: [0.0, 0, 0, 0])      # category -> [iou, tp, fp, fn]


def pq_average(stat, categories, isthing):
    """PQStat.pq_average of eval_vpq_vspw.py:48-74 (categories: dict id -> info, in the GT JSON's order)."""
    pq, sq, rq, n = 0, 0, 0, 0
    per_class = {}
    for label, info in categories.items():
        if isthing is not None and isthing != (info["isthing"] == 1):
            continue
        iou, tp, fp, fn = stat[label] if label in stat else (0.0, 0, 0, 0)
        if tp + fp + fn == 0:
            per_class[label] = {"pq": 0.0, "sq": 0.0, "rq": 0.0, "iou": 0.0, "tp": 0, "fp": 0, "fn": 0}
            continue
        n += 1
        pq_class = iou / (tp + 0.5 * fp + 0.5 * fn)
        sq_class = iou / tp if tp != 0 else 0
        rq_class = tp / (tp + 0.5 * fp + 0.5 * fn)
        per_class[label] = {"pq": pq_class, "sq": sq_class, "rq": rq_class, "iou": iou, "tp": tp, "fp": fp, "fn": fn}
        pq += pq_class
        sq += sq_class
        rq += rq_class
    if n == 0:          # the reference divides by zero here; report zeros instead
        return {"pq": 0.0, "sq": 0.0, "rq": 0.0, "n": 0}, per_class
    return {"pq": pq / n, "sq": sq / n, "rq": rq / n, "n": n}, per_class


class VPQ:
    """Video panoptic quality over window lengths `nframes` (eval_vpq_vspw.py).  update() once per video, in video order."""

    def __init__(self, categories, nframes=VPQ_NFRAMES):
        self.categories = _categories(categories)
        self.nframes = tuple(nframes)
        self.videos = []            # per video: {nframes: {category: [iou, tp, fp, fn]}}

    def update(self, gt_map, pred_map, gt: PanopticGT, pred: PanopticPred, hist=None):
        if hist is None:
            hist = pair_hist(gt_map, pred_map, gt, pred.num_pred)
        self.videos.append(self.video_stats(hist, gt, pred))

    def video_stats(self, hist, gt: PanopticGT, pred: PanopticPred):
        """One video's {nframes: {category: [iou, tp, fp, fn]}} from its pair counts (what update() appends)."""
        return {nf: dict(s) for nf, s in vpq_video_stats(hist, gt, pred, self.categories, self.nframes).items()}

    def state(self):
        return [{nf: dict(s) for nf, s in v.items()} for v in self.videos]

    def result(self, videos=None):
        videos = self.videos if videos is None else videos
        out = {}
        for nf in self.nframes:
            total = _new_pq_stat()
            for v in videos:                         # PQStat.__iadd__ in video order
                for label, (iou, tp, fp, fn) in v[nf].items():
                    s = total[label]
                    s[0] += iou
                    s[1] += tp
                    s[2] += fp
                    s[3] += fn
            res = {}
            for name, isthing in (("All", None), ("Things", True), ("Stuff", False)):
                res[name], per_class = pq_average(total, self.categories, isthing)
                if name == "All":
                    res["per_class"] = per_class
            out[nf] = res
        k = len(self.nframes)
        final = {key: sum(100 * out[nf][name]["pq"] for nf in self.nframes) / k
                 for key, name in (("vpq_all", "All"), ("vpq_thing", "Things"), ("vpq_stuff", "Stuff"))}
        return {"per_nframes": out, **final}


def _categories(categories):
    if isinstance(categories, dict):
        return {int(k): v for k, v in categories.items()}
    return {int(el["id"]): el for el in categories}


def vpq_video_stats(hist, gt: PanopticGT, pred: PanopticPred, categories, nframes=VPQ_NFRAMES):
    """vpq_compute_single_core (eval_vpq_vspw.py:77-216) for every window length, from the per-frame pair counts."""
    T, R, P = hist.shape
    ng = R - 2
    present = hist.sum(1) > 0                                                   # (T, Np + 1)
    present[:, 0] = False
    listed = present if pred.listed is None else pred.listed.copy()
    listed[:, 0] = False
    for t in range(T):                                                          # the prediction checks, :113-127
        extra = np.nonzero(present[t] & ~listed[t])[0]
        if len(extra):
            raise KeyError(f"Segment with ID {int(extra[0])} is presented in PNG and not presented in JSON.")
        missing = np.nonzero(listed[t] & ~present[t])[0]
        if len(missing):
            raise KeyError(f"The following segment IDs {missing.tolist()} are presented in JSON and not presented in PNG.")
    for d in np.nonzero(listed.any(0))[0]:
        if int(pred.category[d]) not in categories:
            raise KeyError(f"Segment with ID {int(d)} has unknown category_id {int(pred.category[d])}.")
    prefix = np.concatenate([np.zeros((1, R, P), np.int64), np.cumsum(hist, 0, dtype=np.int64)])
    area_prefix = np.concatenate([np.zeros((1, ng), np.int64), np.cumsum(gt.area, 0, dtype=np.int64)])
    gcat, pcat = gt.category, pred.category
    crowd = gt.iscrowd == 1
    out = {}
    for nf in nframes:
        stat = _new_pq_stat()
        if T - nf + 1 <= 0:
            out[nf] = stat
            continue
        g_in, p_in = _window_any(gt.listed, nf), _window_any(listed, nf)
        for i in range(T - nf + 1):
            inter = prefix[i + nf] - prefix[i]                                  # (Ng + 2, Np + 1) tube intersections
            ga = area_prefix[i + nf] - area_prefix[i]                           # JSON areas of the GT tubes
            pa = inter.sum(0)                                                   # PNG areas of the predicted tubes
            gi, pi = g_in[i], p_in[i]
            void = inter[0]
            seg = inter[1:ng + 1]                                               # rows of listed ids
            cand = (seg > 0) & gi[:, None] & pi[None, :] & ~crowd[:, None] & (gcat[:, None] == pcat[None, :])
            g_matched = np.zeros(ng, bool)
            p_matched = np.zeros(P, bool)
            for r, p in zip(*np.nonzero(cand)):                                 # np.unique order: (gt id, pred id)
                it = int(seg[r, p])
                union = int(pa[p]) + int(ga[r]) - it - int(void[p])
                iou = it / union
                assert iou <= 1.0, "INVALID IOU VALUE : %d" % int(gt.table[r])
                if iou > 0.5:
                    s = stat[int(gcat[r])]
                    s[1] += 1
                    s[0] += iou
                    g_matched[r] = True
                    p_matched[p] = True
            crowd_rows = {}
            rows = np.nonzero(gi)[0]
            for r in rows[np.lexsort((_first_pos(gt, i, nf, rows), _first_frame(gt.listed, i, nf, rows)))]:
                if g_matched[r]:
                    continue
                if crowd[r]:
                    crowd_rows[int(gcat[r])] = r                                # the last one of a category wins, as there
                    continue
                stat[int(gcat[r])][3] += 1
            for p in np.nonzero(pi)[0]:
                if p_matched[p]:
                    continue
                it = int(void[p])
                c = int(pcat[p])
                if c in crowd_rows:
                    it += int(seg[crowd_rows[c], p])
                if it / int(pa[p]) > 0.5:
                    continue
                stat[c][2] += 1
        out[nf] = stat
    return out


def _first_frame(listed, i, nf, rows):
    w = listed[i:i + nf, rows]
    return np.argmax(w, 0)


def _first_pos(gt, i, nf, rows):
    f = _first_frame(gt.listed, i, nf, rows) + i
    return gt.pos[f, rows]


def write_vpq_txt(path, res):
    """vpq-<k>.txt exactly as eval_vpq_vspw.py:238-251 writes it."""
    metrics = [("All", None), ("Things", True), ("Stuff", False)]
    with open(path, "w") as f:
        f.write("================================================\n")
        f.write("{:10s}| {:>5s}  {:>5s}  {:>5s} {:>5s}".format("", "PQ", "SQ", "RQ", "N\n"))
        f.write("-" * (10 + 7 * 4) + '\n')
        for name, _ in metrics:
            f.write("{:10s}| {:5.1f}  {:5.1f}  {:5.1f} {:5d}\n".format(name, 100 * res[name]['pq'], 100 * res[name]['sq'],
                                                                      100 * res[name]['rq'], res[name]['n']))
        f.write("{:4s}| {:>5s} {:>5s} {:>5s} {:>6s} {:>7s} {:>7s} {:>7s}\n".format("IDX", "PQ", "SQ", "RQ", "IoU", "TP", "FP",
                                                                                   "FN"))
        for idx, r in res['per_class'].items():
            f.write("{:4d} | {:5.1f} {:5.1f} {:5.1f} {:6.1f} {:7d} {:7d} {:7d}\n".format(
                idx, 100 * r['pq'], 100 * r['sq'], 100 * r['rq'], r['iou'], r['tp'], r['fp'], r['fn']))


def write_vpq_final(path, result):
    with open(path, "w") as f:
        f.write("vpq_all:%.4f\n" % result["vpq_all"])
        f.write("vpq_thing:%.4f\n" % result["vpq_thing"])
        f.write("vpq_stuff:%.4f\n" % result["vpq_stuff"])


# ----------------------------------------------------------------------------------------------------------------------------
# STQ
# ----------------------------------------------------------------------------------------------------------------------------
class STQ:
    """Segmentation and tracking quality (segmentation_and_tracking_quality.py) with eval_stq_vspw.py's arguments.  A pixel's
    semantic / instance label is its segment's category / order of first appearance in the video's JSON (255 / 255 where no
    listed segment covers it); instance 0 of a thing class is `crowd` there, and so here."""

    def __init__(self, things, num_classes=124, ignore_label=255, label_bit_shift=16, offset=2 ** 24):
        self.num_classes, self.ignore_label = num_classes, ignore_label
        self.shift, self.offset = label_bit_shift, offset
        self.things = np.array(sorted(int(t) for t in things), dtype=np.int64)
        if offset < num_classes << label_bit_shift:
            raise ValueError("STQ offset too small")
        if ignore_label >= num_classes:
            self.size, self.include = num_classes + 1, np.arange(num_classes)
        else:
            self.size, self.include = num_classes, np.array([i for i in range(num_classes) if i != ignore_label])
        self.seqs = collections.OrderedDict()       # sequence id -> (confusion, gts, preds, intersections, length)

    def update(self, gt_map, pred_map, gt: PanopticGT, pred: PanopticPred, sequence_id, hist=None):
        if hist is None:
            hist = pair_hist(gt_map, pred_map, gt, pred.num_pred)
        self.seqs[sequence_id] = self.sequence_stats(hist, gt, pred, self.seqs.get(sequence_id))

    def sequence_stats(self, hist, gt: PanopticGT, pred: PanopticPred, prev=None):
        """One sequence's (confusion, gts, preds, intersections, length) from its pair counts, added to `prev`."""
        return stq_sequence_stats(hist, gt, pred, self.things, self.size, self.num_classes, self.ignore_label, self.shift,
                                  self.offset, prev)

    def state(self):
        return list(self.seqs.items())

    def result(self, seqs=None):
        seqs = self.seqs if seqs is None else collections.OrderedDict(seqs)
        n = len(seqs)
        num_tubes, aq_per_seq, iou_per_seq, id_per_seq = [0] * n, [0] * n, [0] * n, [''] * n
        for index, (sid, (_, gts, preds, inters, _)) in enumerate(seqs.items()):
            outer_sum = 0.0
            num_tubes[index] = len(gts)
            id_per_seq[index] = sid
            for gt_id, gt_size in gts.items():
                inner_sum = 0.0
                for pr_id, pr_size in preds.items():
                    key = self.offset * gt_id + pr_id
                    if key in inters:
                        tpa = inters[key]
                        fpa = pr_size - tpa
                        fna = gt_size - tpa
                        inner_sum += tpa * (tpa / (tpa + fpa + fna))
                outer_sum += 1.0 / gt_size * inner_sum
            aq_per_seq[index] = outer_sum
        aq_mean = np.sum(aq_per_seq) / np.maximum(np.sum(num_tubes), _EPSILON)
        aq_per_seq = aq_per_seq / np.maximum(num_tubes, _EPSILON)
        total = np.zeros((self.size, self.size), dtype=np.int64)
        for index, (conf, *_rest) in enumerate(seqs.values()):
            conf = conf.copy()
            removal = np.zeros_like(conf)
            removal[self.include, :] = 1.0
            conf *= removal
            total += conf
            inter = conf.diagonal()
            unions = inter + (conf.sum(axis=0) - inter) + (conf.sum(axis=1) - inter)
            ious = inter.astype(np.double) / np.maximum(unions, 1e-15).astype(np.double)
            iou_per_seq[index] = np.sum(ious) / np.count_nonzero(unions)
        inter = total.diagonal()
        unions = inter + (total.sum(axis=0) - inter) + (total.sum(axis=1) - inter)
        ious = inter.astype(np.double) / np.maximum(unions, _EPSILON).astype(np.double)
        iou_mean = np.sum(ious) / np.count_nonzero(unions)
        return {"STQ": np.sqrt(aq_mean * iou_mean), "AQ": aq_mean, "IoU": float(iou_mean),
                "STQ_per_seq": np.sqrt(aq_per_seq * iou_per_seq), "AQ_per_seq": aq_per_seq, "IoU_per_seq": iou_per_seq,
                "ID_per_seq": id_per_seq, "Length_per_seq": [s[4] for s in seqs.values()]}


def _add_stats(d, keys, counts):
    """_update_dict_stats: keys in ascending order, only those that occur."""
    agg = {}
    for k, c in zip(keys.tolist(), counts.tolist()):
        if c:
            agg[k] = agg.get(k, 0) + c
    for k in sorted(agg):
        d[k] = d.get(k, 0) + agg[k]


def stq_sequence_stats(hist, gt: PanopticGT, pred: PanopticPred, things, size, num_classes, ignore_label, shift, offset,
                       prev=None):
    """STQuality.update_state over a video's frames, from its per-frame pair counts."""
    T, R, P = hist.shape
    ng = R - 2
    present = hist.sum(1) > 0
    listed, pinst = pred.resolve(present)
    if prev is None:
        conf, gts, preds, inters, length = np.zeros((size, size), np.int64), {}, {}, {}, 0
    else:
        conf, gts, preds, inters, length = prev
    for t in range(T):
        gsem = np.full(R, 255, np.int64)
        ginst = np.full(R, 255, np.int64)
        lt = gt.listed[t]
        gsem[1:ng + 1][lt] = gt.category[lt]
        ginst[1:ng + 1][lt] = gt.inst[lt]
        psem = np.where(listed[t], pred.category, 255)
        pinst_t = np.where(listed[t], pinst, 255)
        y_true = (gsem << shift) + ginst
        y_pred = (psem << shift) + pinst_t
        sl, sp = gsem.copy(), psem.copy()
        if ignore_label > num_classes:
            sl[sl == ignore_label] = num_classes
            sp[sp == ignore_label] = num_classes
        if (sl >= size).any() or (sp >= size).any() or (sl < 0).any() or (sp < 0).any():
            raise IndexError("STQ: a category id outside the confusion matrix")
        np.add.at(conf, (sl[:, None].repeat(P, 1), sp[None, :].repeat(R, 0)), hist[t])
        thing_g = np.isin(gsem, things)
        thing_p = np.isin(psem, things)
        is_crowd = thing_g & ((y_true & ((1 << shift) - 1)) == 0)
        label_mask = thing_g & ~is_crowd
        h = hist[t]
        _add_stats(preds, y_pred[thing_p], h[~is_crowd][:, thing_p].sum(0))
        _add_stats(gts, y_true[label_mask], h[label_mask].sum(1))
        sub = h[label_mask][:, thing_p]
        keys = (y_true[label_mask][:, None] * offset + y_pred[thing_p][None, :]).reshape(-1)
        _add_stats(inters, keys, sub.reshape(-1))
        length += 1
    return conf, gts, preds, inters, length


# ----------------------------------------------------------------------------------------------------------------------------
# VSS: mIoU and VC
# ----------------------------------------------------------------------------------------------------------------------------
class SemSegConfusion:
    """Evaluator(num_class) of eval_miou_vspw.py: the confusion summed over every frame, then the same float64 expressions."""

    def __init__(self, num_class=124):
        self.num_class = num_class
        self.counts = np.zeros((num_class, num_class), dtype=np.int64)

    def update(self, gt, pred, conf=None):
        if conf is None:
            conf = Fn.sem_confusion(gt, pred, self.num_class).cpu().numpy()
        self.counts += conf

    def state(self):
        return self.counts

    def result(self, counts=None, beforeval=False):
        cm = (self.counts if counts is None else counts).astype(np.float64)
        if beforeval:                                  # Evaluator.beforeval (the script does not call it)
            cm = cm * (np.sum(cm, axis=1) > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = np.diag(cm).sum() / cm.sum()
            acc_class = np.nanmean(np.diag(cm) / cm.sum(axis=1))
            iou = np.diag(cm) / (np.sum(cm, axis=1) + np.sum(cm, axis=0) - np.diag(cm))
            isval = np.sum(cm, axis=1) > 0
            miou = np.nansum(iou * isval) / isval.sum()
            freq = np.sum(cm, axis=1) / np.sum(cm)
            fwiou = (freq[freq > 0] * iou[freq > 0]).sum()
        return {"Acc": acc, "Acc_class": acc_class, "mIoU": miou, "fwIoU": fwiou}


class VideoConsistency:
    """VC_k of eval_vc_vspw.py: per window start i < T - k (videos with T <= k skipped) the fraction of GT-constant pixels
    whose prediction is constant too; VC_k = nanmean over all windows of all videos.  The reference script never clears its
    list between k = 8 and k = 16, so the VC16 it prints is the nanmean over the windows of BOTH lengths: result() reports
    that as VC<k> (the number MODEL_ZOO quotes) and the windows of length k alone as VC<k>_k_only."""

    def __init__(self, ks=(8, 16)):
        self.ks = tuple(int(k) for k in ks)
        self.videos = []            # per video: (gt_const, both_const), each (len(ks), T)

    def update(self, gt, pred, counts=None):
        if counts is None:
            gc, bc = Fn.video_consistency(gt, pred, self.ks)
            counts = (gc.cpu().numpy(), bc.cpu().numpy())
        self.videos.append(counts)

    def state(self):
        return self.videos

    def accs(self, videos=None):
        """{k: [acc of every window, videos in order]} as get_common returns them."""
        videos = self.videos if videos is None else videos
        out = {}
        for j, k in enumerate(self.ks):
            accs = []
            for gc, bc in videos:
                T = gc.shape[1]
                if T <= k:
                    continue
                with np.errstate(divide="ignore", invalid="ignore"):
                    accs.extend((bc[j, :T - k] / gc[j, :T - k]).tolist())
            out[k] = accs
        return out

    def result(self, videos=None):
        accs = self.accs(videos)
        res, running = {}, []
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for k in self.ks:
                running.extend(accs[k])
                res[f"VC{k}"] = np.nanmean(np.array(running))
                res[f"VC{k}_k_only"] = np.nanmean(np.array(accs[k]))
        return res


# ----------------------------------------------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------------------------------------------
def _png(path, rgb_id=False):
    from PIL import Image
    a = np.array(Image.open(path))
    if rgb_id:
        a = a.astype(np.int32)
        return a[:, :, 0] + a[:, :, 1] * 256 + a[:, :, 2] * 65536
    return a


def _decode(paths, rgb_id, pool):
    return np.stack(list(pool.map(lambda p: _png(p, rgb_id), paths)))


def _device(name):
    if name == "auto":
        return "cuda" if torch.cuda.is_available() else "cpu"
    return name


def map_pred_ids(pred_raw, raw_table, strict):
    """Raw predicted ids (T, H, W) -> dense ids through the sorted table (dense d = table[d - 1]; 0 stays 0).  An id that the
    table does not list becomes len(table) + 1 when `strict` (pan_pair_hist then raises: the reference's KeyError) and 0
    otherwise (the STQ script leaves such pixels unlabelled)."""
    tb = torch.as_tensor(raw_table, dtype=torch.int64, device=pred_raw.device)
    p = pred_raw.long()
    if len(raw_table) == 0:
        dense = torch.zeros_like(p)
        found = torch.zeros_like(p, dtype=torch.bool)
    else:
        pos = torch.searchsorted(tb, p).clamp_(max=len(raw_table) - 1)
        found = tb[pos] == p
        dense = pos + 1
    other = len(raw_table) + 1 if strict else 0
    return torch.where(found, dense, torch.where(p == 0, torch.zeros_like(p), torch.full_like(p, other))).to(torch.int32)


def _load_vipseg(args):
    with open(os.path.join(args.submit_dir, "pred.json")) as f:
        pred_j = {a["video_id"]: a["annotations"] for a in json.load(f)["annotations"]}
    with open(args.pan_gt_json_file) as f:
        gt_json = json.load(f)
    gt_j = {a["video_id"]: a["annotations"] for a in gt_json["annotations"]}
    return gt_json, gt_j, pred_j


def _vipseg_videos(args, loaded, device, strict, pool):
    """Yield (video_id, gt_map, pred_map, PanopticGT, PanopticPred) in the GT JSON's video order."""
    gt_json, gt_j, pred_j = loaded
    for video in gt_json["videos"]:
        vid = video["video_id"]
        names = [im["file_name"] for im in video["images"]]
        gt_js, pred_js = gt_j[vid], pred_j[vid]
        assert len(gt_js) == len(pred_js)
        gt_map = torch.from_numpy(_decode([os.path.join(args.truth_dir, vid, n) for n in names], True, pool))
        pred_raw = torch.from_numpy(_decode([os.path.join(args.submit_dir, "pan_pred", vid, n) for n in names], True, pool))
        pred, raw_table = PanopticPred.from_json(pred_js)
        yield vid, gt_map.to(device), map_pred_ids(pred_raw.to(device), raw_table, strict), PanopticGT(gt_js), pred


def _cmd_vpq(args):
    device = _device(args.device)
    loaded = _load_vipseg(args)
    vpq = VPQ(loaded[0]["categories"])
    with ThreadPoolExecutor(MAX_DECODE_THREADS) as pool:
        for vid, gt_map, pred_map, gt, pred in _vipseg_videos(args, loaded, device, True, pool):
            try:
                hist = pair_hist(gt_map, pred_map, gt, pred.num_pred)
            except ValueError:
                raise KeyError(f"video {vid}: a segment ID is presented in PNG and not presented in JSON.") from None
            vpq.update(None, None, gt, pred, hist=hist)
    res = vpq.result()
    for nf in vpq.nframes:
        r = res["per_nframes"][nf]
        write_vpq_txt(os.path.join(args.submit_dir, "vpq-%d.txt" % ((nf - 1) * 5)), r)
        print(100 * r["All"]["pq"], 100 * r["Things"]["pq"], 100 * r["Stuff"]["pq"])
    write_vpq_final(os.path.join(args.submit_dir, "vpq-final.txt"), res)
    return res


def _cmd_stq(args):
    device = _device(args.device)
    loaded = _load_vipseg(args)
    stq = STQ([c["id"] for c in loaded[0]["categories"] if c["isthing"]], **STQ_ARGS)
    with ThreadPoolExecutor(MAX_DECODE_THREADS) as pool:
        for seq_id, (vid, gt_map, pred_map, gt, pred) in enumerate(_vipseg_videos(args, loaded, device, False, pool)):
            stq.update(gt_map, pred_map, gt, pred, seq_id)
    r = stq.result()
    print('*' * 100)
    print('STQ : {}'.format(r['STQ']))
    print('AQ :{}'.format(r['AQ']))
    print('IoU:{}'.format(r['IoU']))
    print('STQ_per_seq')
    print(r['STQ_per_seq'])
    print('AQ_per_seq')
    print(r['AQ_per_seq'])
    print('ID_per_seq')
    print(r['ID_per_seq'])
    print('Length_per_seq')
    print(r['Length_per_seq'])
    print('*' * 100)
    return r


def _vspw_list(root):
    with open(os.path.join(root, "val.txt")) as f:
        return [line[:-1] for line in f.readlines()]


def _cmd_miou(args):
    device = _device(args.device)
    ev = SemSegConfusion(124)
    with ThreadPoolExecutor(MAX_DECODE_THREADS) as pool:
        for video in _vspw_list(args.dir):
            names = os.listdir(os.path.join(args.dir, "data", video, "mask"))
            if not names:
                continue
            gt = _decode([os.path.join(args.dir, "data", video, "mask", n) for n in names], False, pool)
            pred = _decode([os.path.join(args.pred, video, n) for n in names], False, pool)
            ev.update(torch.from_numpy(gt.astype(np.int32)).to(device), torch.from_numpy(pred.astype(np.int32)).to(device))
    r = ev.result()
    print("Acc:{}, Acc_class:{}, mIoU:{}, fwIoU: {}".format(r["Acc"], r["Acc_class"], r["mIoU"], r["fwIoU"]))
    return r


def _cmd_vc(args):
    device = _device(args.device)
    vc = VideoConsistency((8, 16))
    split = "val.txt"
    with ThreadPoolExecutor(MAX_DECODE_THREADS) as pool:
        for video in _vspw_list(args.dir):
            names = sorted(os.listdir(os.path.join(args.dir, "data", video, "mask")))
            if len(names) <= min(vc.ks):
                continue
            gt = _decode([os.path.join(args.dir, "data", video, "mask", n) for n in names], False, pool)
            pred = _decode([os.path.join(args.pred, video, n) for n in names], False, pool)
            vc.update(torch.from_numpy(gt.astype(np.int32)).to(device), torch.from_numpy(pred.astype(np.int32)).to(device))
    r = vc.result()
    for j, k in enumerate(vc.ks):
        for gc, bc in vc.videos:
            T = gc.shape[1]
            if T <= k:
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                a = (bc[j, :T - k] / gc[j, :T - k]).tolist()
            print(sum(a) / len(a))
        print(args.pred)
        print('*' * 10)
        print('VC{} score: {} on {} set'.format(k, r[f"VC{k}"], split))
        print('*' * 10)
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m dvis_plus_amd.video_metrics", description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="metric", required=True)
    for name in ("vpq", "stq"):
        s = sub.add_parser(name)
        s.add_argument("--submit_dir", "-i", required=True)
        s.add_argument("--truth_dir", required=True)
        s.add_argument("--pan_gt_json_file", required=True)
        s.add_argument("--num_processes", type=int, default=8, help="accepted for compatibility; unused")
    for name in ("miou", "vc"):
        s = sub.add_parser(name)
        s.add_argument("dir", help="VSPW root (val.txt, data/<video>/mask/*.png)")
        s.add_argument("pred", help="prediction root (<video>/<frame>.png)")
    for s in sub.choices.values():
        s.add_argument("--device", default="auto", help="cuda | cpu | auto (default)")
    args = ap.parse_args(argv)
    return {"vpq": _cmd_vpq, "stq": _cmd_stq, "miou": _cmd_miou, "vc": _cmd_vc}[args.metric](args)


if __name__ == "__main__":
    main(sys.argv[1:])
