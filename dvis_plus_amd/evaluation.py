"""detectron2-protocol evaluators that SCORE video panoptic / semantic segmentation (VPQ + STQ, mIoU + VC) on the device.

The reference's VPSEvaluator / VSSEvaluator (dvis_Plus/data_video/vps_eval.py, vss_eval.py) only write PNG + JSON predictions,
one segment mask and bbox at a time; the numbers then come from the offline scripts in utils/.  These take the same constructor
(`(dataset_name, cfg, distributed, output_dir)`, train_net_video.py:83) and the reset / process / evaluate protocol, read the
ground truth themselves and return the scripts' final numbers from evaluate():

    VPSEvaluator -> {"vpq": {"vpq_all", "vpq_thing", "vpq_stuff", "per_nframes"}, "stq": {"STQ", "AQ", "IoU", ...}}
    VSSEvaluator -> {"sem_seg": {"mIoU", "Acc", "Acc_class", "fwIoU", "VC8", "VC16", "VC16_k_only", ...}}

process() accepts the product's device outputs or their `to_reference_format` CPU form (copied to the device).  Per-video
statistics are kept with the video's position in the dataset, gathered over torch.distributed in evaluate() and reduced in
video order, so a run on N ranks gives the numbers of a run on one.  d2.install() does not register these classes.

The writers of the files the VIPSeg / VSPW evaluation servers take (VPSPredictionWriter, VSSPredictionWriter, for test splits
without ground truth) live in pred_writers.py and are re-exported here.
"""
import json
import os

import numpy as np
import torch

from . import video_metrics as VM


def _metadata(dataset_name, needed):
    """detectron2's registered metadata of `dataset_name`; raises when it is needed (a keyword override is missing) and
    detectron2 is not importable."""
    try:
        from detectron2.data import MetadataCatalog
    except ImportError:
        raise RuntimeError(f"{dataset_name}: detectron2 is not importable, so the dataset metadata is unavailable; "
                           f"pass {needed} explicitly") from None
    return MetadataCatalog.get(dataset_name)


def _gather(obj, distributed):
    import torch.distributed as dist
    if not (distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return [obj]
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, obj)
    return out


def _device(outputs_map, device):
    if device is not None:
        return torch.device(device)
    if outputs_map.is_cuda:
        return outputs_map.device
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def _frame_stems(inputs0):
    names = [inputs0["file_names"][i] for i in inputs0.get("frame_idx", range(len(inputs0["file_names"])))]
    return [os.path.splitext(os.path.basename(n))[0] for n in names]


class VPSEvaluator:
    """VPQ (utils/eval_vpq_vspw.py) and STQ (utils/eval_stq_vspw.py) of the product's panoptic maps.

    Ground truth: the dataset's registered `panoptic_root` / `panoptic_json` (dvis_Plus/data_video/datasets/vps.py:112-115), or
    the keyword overrides.  Category ids: contiguous -> dataset ids as vps_eval.py:79-86,114-119 (things first, then stuff),
    from the metadata's thing / stuff_dataset_id_to_contiguous_id or the `thing_dataset_ids` / `stuff_dataset_ids` overrides."""

    def __init__(self, dataset_name, cfg=None, distributed=True, output_dir=None, *, panoptic_root=None, panoptic_json=None,
                 thing_dataset_ids=None, stuff_dataset_ids=None, device=None):
        meta = None
        if None in (panoptic_root, panoptic_json, thing_dataset_ids, stuff_dataset_ids):
            meta = _metadata(dataset_name, "panoptic_root, panoptic_json, thing_dataset_ids and stuff_dataset_ids")
        self.panoptic_root = panoptic_root if panoptic_root is not None else meta.panoptic_root
        panoptic_json = panoptic_json if panoptic_json is not None else meta.panoptic_json
        self.thing_ids = list(thing_dataset_ids if thing_dataset_ids is not None
                              else meta.thing_dataset_id_to_contiguous_id.values())
        self.stuff_ids = list(stuff_dataset_ids if stuff_dataset_ids is not None
                              else meta.stuff_dataset_id_to_contiguous_id.values())
        with open(panoptic_json) as f:
            gt_json = json.load(f)
        self.categories = gt_json["categories"]
        self._vpq = VM.VPQ(self.categories)
        self._stq = VM.STQ([c["id"] for c in self.categories if c["isthing"]], **VM.STQ_ARGS)
        self.video_order = {v["video_id"]: n for n, v in enumerate(gt_json["videos"])}
        self.gt_annotations = {a["video_id"]: a["annotations"] for a in gt_json["annotations"]}
        self._distributed, self._output_dir, self._device = distributed, output_dir, device
        self.reset()

    def reset(self):
        self._videos = []          # (order, vpq stats, stq stats)

    def _dataset_category(self, c):
        c = int(c)
        return self.thing_ids[c] if c < len(self.thing_ids) else self.stuff_ids[c - len(self.thing_ids)]

    def process(self, inputs, outputs):
        assert len(inputs) == 1, "More than one inputs are loaded for inference!"
        video_id = inputs[0]["video_id"]
        pan = outputs["pred_masks"]
        dev = _device(pan, self._device)
        stems = _frame_stems(inputs[0])
        anns = {os.path.splitext(os.path.basename(a["file_name"]))[0]: a for a in self.gt_annotations[video_id]}
        frame_anns = [anns[s] for s in stems]
        gt_map = torch.from_numpy(np.stack([VM._png(os.path.join(self.panoptic_root, video_id, s + ".png"), True)
                                            for s in stems])).to(dev)
        segs = outputs["segments_infos"]
        n = max([int(s["id"]) for s in segs], default=0)
        cat = np.full(n + 1, -1, np.int64)
        for s in segs:
            cat[int(s["id"])] = self._dataset_category(s["category_id"])
        gt = VM.PanopticGT(frame_anns)
        pred = VM.PanopticPred(cat)
        hist = VM.pair_hist(gt_map, pan.to(dev), gt, n)
        self._videos.append((self.video_order[video_id], self._vpq.video_stats(hist, gt, pred),
                             self._stq.sequence_stats(hist, gt, pred)))

    def evaluate(self):
        videos = sorted((v for part in _gather(self._videos, self._distributed) for v in part), key=lambda v: v[0])
        if not videos:
            return {}
        return {"vpq": self._vpq.result([v[1] for v in videos]), "stq": self._stq.result([(v[0], v[2]) for v in videos])}


class VSSEvaluator:
    """mIoU (utils/eval_miou_vspw.py) and VC8 / VC16 (utils/eval_vc_vspw.py) of the product's semantic maps.

    Ground truth: the VSPW masks `<vspw_root>/data/<video>/mask/<frame>.png`, videos ordered as `<vspw_root>/val.txt` lists them.
    vspw_root: the keyword, or the parent of the registered image root (dvis_Plus/data_video/datasets/vss.py registers
    image_root = `<root>/VSPW_480p/data/`, whose `<video>/origin` holds the frames).  Predictions are mapped contiguous -> dataset
    ids and cast to uint8 as vss_eval.py:85-95 does before they are written."""

    def __init__(self, dataset_name, cfg=None, distributed=True, output_dir=None, *, vspw_root=None, dataset_ids=None,
                 ignore_label=None, num_class=124, ks=(8, 16), device=None):
        meta = None
        if vspw_root is None or dataset_ids is None or ignore_label is None:
            meta = _metadata(dataset_name, "vspw_root, dataset_ids and ignore_label")
        if vspw_root is None:
            vspw_root = os.path.dirname(os.path.normpath(meta.image_root))
        self.vspw_root = vspw_root
        ids = list(dataset_ids if dataset_ids is not None else meta.stuff_dataset_id_to_contiguous_id.keys())
        self.ignore = int(ignore_label if ignore_label is not None else meta.ignore_label)
        lut = np.full(256, 255, np.int64)
        for c, d in enumerate(ids[:256]):
            lut[c] = d
        lut[self.ignore] = self.ignore
        self.lut = lut % 256
        order = os.path.join(vspw_root, "val.txt")
        self.video_order = {}
        if os.path.exists(order):
            with open(order) as f:
                self.video_order = {line.strip(): n for n, line in enumerate(f) if line.strip()}
        self.num_class, self.ks = num_class, tuple(ks)
        self._distributed, self._output_dir, self._device = distributed, output_dir, device
        self.reset()

    def reset(self):
        self._videos = []          # (order, confusion, vc counts)

    def process(self, inputs, outputs):
        assert len(inputs) == 1, "More than one inputs are loaded for inference!"
        video_id = inputs[0]["video_id"]
        sem = outputs["pred_masks"]
        dev = _device(sem, self._device)
        stems = _frame_stems(inputs[0])
        order = np.argsort(stems, kind="stable")                 # eval_vc_vspw.py scores the frames in sorted name order
        stems = [stems[i] for i in order]
        gt = torch.from_numpy(np.stack([VM._png(os.path.join(self.vspw_root, "data", video_id, "mask", s + ".png"))
                                        for s in stems]).astype(np.int32)).to(dev)
        lut = torch.as_tensor(self.lut, dtype=torch.int32, device=dev)
        pred = lut[(sem.to(dev).long() & 255)][torch.as_tensor(order, device=dev)]   # astype(uint8), then the id map
        conf = VM.Fn.sem_confusion(gt, pred, self.num_class).cpu().numpy()
        gc, bc = VM.Fn.video_consistency(gt, pred, self.ks)
        key = self.video_order.get(video_id, len(self.video_order))
        self._videos.append((key, video_id, conf, (gc.cpu().numpy(), bc.cpu().numpy())))

    def evaluate(self):
        videos = sorted((v for part in _gather(self._videos, self._distributed) for v in part), key=lambda v: (v[0], v[1]))
        if not videos:
            return {}
        seg = VM.SemSegConfusion(self.num_class)
        res = seg.result(sum(v[2] for v in videos))
        res.update(VM.VideoConsistency(self.ks).result([v[3] for v in videos]))
        return {"sem_seg": res}


class YTVISEvaluator:
    """YouTube-VIS / OVIS evaluation (dvis_Plus/data_video/ytvis_eval.py) with the pixel work on the device.

    Same constructor and protocol as the reference (`(dataset_name, tasks=None, distributed=True, output_dir=None, *,
    use_fast_impl=True)`, train_net_video.py passes cfg as `tasks`; use_fast_impl is accepted and ignored, as there).  The dataset
    JSON, the dataset -> contiguous category ids and the class names come from the registered metadata (`json_file`,
    `thing_dataset_id_to_contiguous_id`, `thing_classes`) or the keyword overrides.

    process() RLE-encodes the predicted masks on the device and keeps only the strings, scores, labels and areas; when the JSON
    has annotations it also decodes the video's ground truth there and keeps the (P, G) intersection table.  evaluate() writes
    instances_predictions.pth and results.json exactly as the reference does (the latter byte-identical: it is what the YTVIS /
    OVIS evaluation servers take) and returns {"segm": {AP, AP50, ..., AR10, AP-<class>}} when there are annotations, else {}."""

    def __init__(self, dataset_name, tasks=None, distributed=True, output_dir=None, *, use_fast_impl=True, json_file=None,
                 dataset_id_to_contiguous_id=None, class_names=None, device=None):
        from . import vis_metrics as VIS
        meta = None
        if json_file is None or dataset_id_to_contiguous_id is None:
            meta = _metadata(dataset_name, "json_file and dataset_id_to_contiguous_id")
        if json_file is None:
            json_file = meta.json_file
        if dataset_id_to_contiguous_id is None and hasattr(meta, "thing_dataset_id_to_contiguous_id"):
            dataset_id_to_contiguous_id = meta.thing_dataset_id_to_contiguous_id
        if class_names is None and meta is not None:
            class_names = meta.get("thing_classes")
        self._id_map = dict(dataset_id_to_contiguous_id) if dataset_id_to_contiguous_id is not None else None
        self._class_names = class_names
        self._gt = VIS.YTVISGroundTruth(json_file)
        self._do_evaluation = self._gt.has_annotations
        self._distributed, self._output_dir, self._device = distributed, output_dir, device
        self.reset()

    def reset(self):
        self._videos = []          # (prediction dicts, per-frame areas (P, T), I (P, G) or None, GT area totals, scored frames)

    def process(self, inputs, outputs):
        from . import functions as Fn
        from . import vis_metrics as VIS
        assert len(inputs) == 1, "More than one inputs are loaded for inference!"
        video_id = inputs[0]["video_id"]
        scores, labels, masks = outputs["pred_scores"], outputs["pred_labels"], outputs["pred_masks"]
        scores = scores.tolist() if torch.is_tensor(scores) else [float(s) for s in scores]
        labels = labels.tolist() if torch.is_tensor(labels) else [int(x) for x in labels]
        if not torch.is_tensor(masks):
            masks = torch.stack(list(masks)) if len(masks) else torch.zeros((0, 0, 1, 1), dtype=torch.bool)
        dev = _device(masks, self._device)
        masks = masks.to(dev)
        P = len(scores)
        if P == 0:
            return
        T, H, W = masks.shape[1:]
        v = self._gt.videos.get(video_id)
        if v is not None and (v["height"], v["width"]) != (H, W):
            raise ValueError(f"video {video_id}: predicted masks are {H} x {W}, the dataset says {v['height']} x {v['width']}")
        runs, run_off, area = Fn.rle_encode(masks.reshape(P * T, H, W))
        chars, str_off = Fn.rle_strings(runs, run_off)
        chars, str_off = chars.cpu().numpy().tobytes(), str_off.cpu().tolist()
        area = area.view(P, T).cpu().numpy()
        preds = []
        for p in range(P):
            segms = [{"size": [H, W], "counts": chars[str_off[p * T + t]:str_off[p * T + t + 1]].decode("ascii")}
                     for t in range(T)]
            preds.append({"video_id": video_id, "score": scores[p], "category_id": labels[p], "segmentations": segms})
        I = ga = None
        frames = T
        if self._do_evaluation:
            if v is None:
                raise ValueError(f"video {video_id} is not in the dataset")
            I, ga = VIS.intersections(self._gt, video_id, masks)
            frames = min([T] + [len(a["segmentations"]) for a in self._gt.anns.get(video_id, [])])
        self._videos.append((preds, area, I, ga, frames))

    def evaluate(self):
        import torch.distributed as dist
        from . import vis_metrics as VIS
        videos = [v for part in _gather(self._videos, self._distributed) for v in part]     # rank order, as comm.gather
        predictions = [d for v in videos for d in v[0]]
        if len(predictions) == 0:
            return {}
        main = not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0
        if self._output_dir and main:
            os.makedirs(self._output_dir, exist_ok=True)
            torch.save(predictions, os.path.join(self._output_dir, "instances_predictions.pth"))
        if self._id_map is not None:
            contiguous = list(self._id_map.values())
            num_classes = len(contiguous)
            assert min(contiguous) == 0 and max(contiguous) == num_classes - 1
            reverse = {c: d for d, c in self._id_map.items()}
            unmapped = []
            for r in predictions:
                assert r["category_id"] < num_classes, (f"A prediction has class={r['category_id']}, but the dataset only has "
                                                        f"{num_classes} classes")
                unmapped.append(dict(r, category_id=reverse[r["category_id"]]))
            predictions = unmapped
        if self._output_dir and main:
            with open(os.path.join(self._output_dir, "results.json"), "w") as f:
                f.write(json.dumps(predictions))
        if not self._do_evaluation:
            return {}
        dets, tables, n = [], {}, 0
        for preds, area, I, ga, frames in videos:
            vid = preds[0]["video_id"]
            idx = list(range(n, n + len(preds)))
            for p, r in enumerate(predictions[n:n + len(preds)]):
                dets.append(VIS.Detection(vid, r["category_id"], r["score"], area[p], n + p + 1))
            tables[vid] = VIS.VideoTable(idx, I, area[:, :frames].sum(1), ga)
            n += len(preds)
        return {"segm": VIS.derive_results(VIS.evaluate(self._gt, dets, tables), self._class_names)}


from .pred_writers import PanopticIdGenerator, VPSPredictionWriter, VSSPredictionWriter  # noqa: E402,F401  (re-export)
