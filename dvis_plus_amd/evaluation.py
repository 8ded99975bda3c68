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
