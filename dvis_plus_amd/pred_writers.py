"""detectron2-protocol writers of the VIPSeg / VSPW prediction files that the evaluation servers take, from device outputs.

The reference's VPSEvaluator / VSSEvaluator (dvis_Plus/data_video/vps_eval.py, vss_eval.py) only write these files: per video
the PNGs of every frame, and for VIPSeg one pred.json at the end.  Here the pixel work runs on the device (csrc/pred_write.hip
through functions.py): one pass gives every segment's per-frame area and bounds, another paints the PNG pixels, and only the
painted uint8 maps and the small stats table travel to the host (pinned buffers).  Pillow encodes the PNGs on a bounded thread
pool while the next video runs; evaluate() drains it.  The files are those of the reference: the same arrays, and with the same
numpy seed byte-identical PNGs and pred.json.

    VPSPredictionWriter -> <output_dir>/pan_pred/<video>/<frame>.png (RGB-encoded segment ids) + <output_dir>/pred.json
    VSSPredictionWriter -> <output_dir>/<video>/<frame>.png (uint8 dataset class ids)

Both return {} from evaluate(), as the reference does; `python -m dvis_plus_amd.video_metrics` scores the trees when the ground
truth exists.  process() accepts the product's device outputs or their `to_reference_format` CPU form (moved to the device when
there is one; `device="cpu"` keeps the work on the CPU formulations of cpu_ops.py).
"""
import logging
import os
import threading
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import functions as Fn

MAX_ENCODE_THREADS = 16        # PNG encoders per writer (zlib releases the GIL); never sized from the machine's CPU count
MAX_VIDEOS_IN_FLIGHT = 2       # videos whose PNGs may still be encoding when the next one is processed


def rgb2id(color):
    """Segment id of an RGB colour: r + 256 g + 65536 b (the VIPSeg PNG encoding)."""
    return int(color[0]) + 256 * int(color[1]) + 65536 * int(color[2])


class PanopticIdGenerator:
    """The colour rule of the VIPSeg prediction PNGs (panopticapi.utils.IdGenerator's behaviour, restated).

    categories: {dataset id: {"isthing": 0 / 1, "color": [r, g, b]}} (the registered metadata's `categories`), or a list of such
    dicts with an "id".  Black and every stuff colour start out taken.
      * a stuff category's segments all get the category colour (two stuff segments of one category share colour and id);
      * a thing category's first segment gets the category colour when it is not taken yet;
      * any later one gets the colour plus np.random.randint(-30, 31, size=3), clipped to [0, 255], redrawn until the colour is
        not taken.
    The draws come from numpy's global generator, so a run seeded like the reference's reproduces its colours."""

    def __init__(self, categories):
        if not isinstance(categories, dict):
            categories = {c["id"]: c for c in categories}
        self.categories = categories
        self.taken = {(0, 0, 0)}
        for c in categories.values():
            if c["isthing"] == 0:
                self.taken.add(tuple(int(x) for x in c["color"]))

    def get_color(self, cat_id):
        cat = self.categories[cat_id]
        base = tuple(int(x) for x in cat["color"])
        if cat["isthing"] == 0:
            return base
        if base not in self.taken:
            self.taken.add(base)
            return base
        while True:
            jitter = np.random.randint(-30, 31, size=3)
            color = tuple(int(x) for x in np.clip(np.asarray(base, np.int64) + jitter, 0, 255))
            if color not in self.taken:
                self.taken.add(color)
                return color

    def get_id(self, cat_id):
        return rgb2id(self.get_color(cat_id))


def _png_stem(name):
    """vps_eval.py:150 / vss_eval.py:106: the file name up to its FIRST dot (a.b.jpg -> a)."""
    return name.split('/')[-1].split('.')[0]


class _PngWriter:
    """Pillow PNG encodes on a bounded thread pool, over frames that stay in a recycled pinned host buffer until written."""

    def __init__(self, threads):
        self.threads = max(1, min(int(threads), MAX_ENCODE_THREADS))
        self._pool = None
        self._videos = deque()          # per video: its futures
        self._free = []                 # pinned uint8 buffers no frame reads any more
        self._lock = threading.Lock()
        self.host_bytes = 0             # device -> host bytes copied so far

    def to_host(self, tensors):
        """Host copies of device tensors (one pinned buffer, one sync); CPU tensors are returned as they are.  The second
        value is the buffer to hand to submit() with the frames that read it."""
        if not tensors[0].is_cuda:
            return [t.contiguous() for t in tensors], None
        sizes = [t.numel() * t.element_size() for t in tensors]
        offs = [0]
        for s in sizes[:-1]:
            offs.append((offs[-1] + s + 63) // 64 * 64)
        total = offs[-1] + sizes[-1]
        buf = self._take(total)
        out = []
        for t, o, s in zip(tensors, offs, sizes):
            h = buf[o:o + s].view(t.dtype).view(t.shape)
            h.copy_(t, non_blocking=True)
            out.append(h)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(tensors[0].device))
        ev.synchronize()
        self.host_bytes += sum(sizes)
        return out, buf

    def _take(self, nbytes):
        with self._lock:
            for i, b in enumerate(self._free):
                if b.numel() >= nbytes:
                    return self._free.pop(i)
        return torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)

    def submit(self, jobs, buf):
        """jobs: (path, (H, W[, 3]) uint8 array); buf goes back to the free list once every job has run.  Of jobs with one path
        only the last is kept (frame names equal up to their first dot: the reference's later save wins)."""
        from PIL import Image
        jobs = list({p: (p, a) for p, a in jobs}.values())
        while len(self._videos) >= MAX_VIDEOS_IN_FLIGHT:
            for f in self._videos.popleft():
                f.result()
        if self._pool is None:
            self._pool = ThreadPoolExecutor(self.threads, thread_name_prefix="png")
        left = [len(jobs)]

        def one(path, arr):
            try:
                Image.fromarray(arr).save(path)
            finally:
                with self._lock:
                    left[0] -= 1
                    if left[0] == 0 and buf is not None:
                        self._free.append(buf)
        self._videos.append([self._pool.submit(one, p, a) for p, a in jobs])
        if not jobs and buf is not None:
            self._free.append(buf)

    def drain(self):
        """Wait for every submitted PNG (raises the first encode error)."""
        while self._videos:
            for f in self._videos.popleft():
                f.result()


class VPSPredictionWriter:
    """VIPSeg prediction files, as dvis_Plus/data_video/vps_eval.py writes them.

    Same constructor as the reference (`(dataset_name, tasks=None, distributed=True, output_dir=None, *, use_fast_impl=True)`;
    tasks and use_fast_impl are accepted and unused there too).  The registered metadata gives `categories` (dataset id -> dict
    with "isthing" and "color") and the thing / stuff_dataset_id_to_contiguous_id maps; the keyword overrides of the same names
    replace it.  As in the reference, contiguous category c of a thing maps to the c-th VALUE of the thing map, and stuff category
    c to the (c - #things)-th value of the stuff map.

    process() writes the video's PNGs (every rank its own) and keeps its annotations; evaluate() waits for the PNGs, gathers the
    annotations to rank 0 in rank order and writes pred.json there.  The reference's quirks are kept: frames are
    file_names[frame_idx]; a PNG is named after the file name up to its first dot; `file_name` in the JSON is the full base name;
    a bbox is [x, y, xmax - x, ymax - y] (no +1); a segment absent from a frame has no entry there; segments_info lists the
    segments in segments_infos order, with `id` = rgb2id(colour)."""

    def __init__(self, dataset_name, tasks=None, distributed=True, output_dir=None, *, use_fast_impl=True, categories=None,
                 thing_dataset_id_to_contiguous_id=None, stuff_dataset_id_to_contiguous_id=None, device=None,
                 encode_threads=MAX_ENCODE_THREADS):
        from .evaluation import _metadata
        self._logger = logging.getLogger(__name__)
        meta = None
        if categories is None or thing_dataset_id_to_contiguous_id is None or stuff_dataset_id_to_contiguous_id is None:
            meta = _metadata(dataset_name, "categories, thing_dataset_id_to_contiguous_id and stuff_dataset_id_to_contiguous_id")
        self.categories = categories if categories is not None else meta.categories
        things = (thing_dataset_id_to_contiguous_id if thing_dataset_id_to_contiguous_id is not None
                  else meta.thing_dataset_id_to_contiguous_id)
        stuff = (stuff_dataset_id_to_contiguous_id if stuff_dataset_id_to_contiguous_id is not None
                 else meta.stuff_dataset_id_to_contiguous_id)
        self.contiguous_id_to_thing_dataset_id = dict(enumerate(things.values()))
        self.contiguous_id_to_stuff_dataset_id = dict(enumerate(stuff.values()))
        self._distributed, self._output_dir, self._device = distributed, output_dir, device
        self._png = _PngWriter(encode_threads)
        self._predictions = []

    @property
    def host_bytes(self):
        """Bytes copied device -> host by process() so far (the painted maps and the stats tables)."""
        return self._png.host_bytes

    def reset(self):
        if self._output_dir is None:
            raise ValueError("VPSPredictionWriter needs an output_dir")
        self._png.drain()
        self._predictions = []
        os.makedirs(os.path.join(self._output_dir, "pan_pred"), exist_ok=True)

    def _dataset_category(self, seg):
        sem = seg["category_id"]
        if seg["isthing"]:
            return self.contiguous_id_to_thing_dataset_id[sem]
        return self.contiguous_id_to_stuff_dataset_id[sem - len(self.contiguous_id_to_thing_dataset_id)]

    def process(self, inputs, outputs):
        from .evaluation import _device
        assert len(inputs) == 1, "More than one inputs are loaded for inference!"
        video_id = inputs[0]["video_id"]
        image_names = [inputs[0]["file_names"][idx] for idx in inputs[0]["frame_idx"]]
        H, W = (int(s) for s in outputs["image_size"])
        pan = outputs["pred_masks"]
        segs = outputs["segments_infos"]
        if pan.dim() != 3 or tuple(pan.shape[1:]) != (H, W) or len(image_names) > pan.shape[0]:
            raise ValueError(f"video {video_id}: pred_masks {tuple(pan.shape)} does not hold {len(image_names)} frames of "
                             f"{H} x {W}")
        pan = pan.to(_device(pan, self._device))
        colors = PanopticIdGenerator(self.categories)
        n = max([int(s["id"]) for s in segs], default=0)
        lut = np.zeros(n + 1, np.int32)
        listed = []
        for s in segs:
            sid = int(s["id"])
            if sid < 0:
                raise ValueError(f"video {video_id}: negative segment id {sid}")
            sem = self._dataset_category(s)
            color = colors.get_color(sem)
            lut[sid] = color[0] | (color[1] << 8) | (color[2] << 16)
            listed.append((sid, int(sem), rgb2id(color)))
        stats, _ = Fn.pan_segment_stats(pan, n)
        rgb = Fn.pan_paint_rgb(pan, torch.from_numpy(lut).to(pan.device))
        (stats, rgb), buf = self._png.to_host([stats, rgb])
        stats, rgb = stats.numpy(), rgb.numpy()
        annotations = []
        for i, image_name in enumerate(image_names):
            infos = []
            for sid, sem, pid in listed:
                area, x0, y0, x1, y1 = (int(v) for v in stats[i, sid])
                if area:
                    infos.append({"bbox": [x0, y0, x1 - x0, y1 - y0], "area": area, "category_id": sem, "iscrowd": 0,
                                  "id": pid})
            annotations.append({"segments_info": infos, "file_name": image_name.split('/')[-1]})
        vdir = os.path.join(self._output_dir, "pan_pred", video_id)
        os.makedirs(vdir, exist_ok=True)
        self._png.submit([(os.path.join(vdir, _png_stem(nm) + ".png"), rgb[i]) for i, nm in enumerate(image_names)], buf)
        self._predictions.append({"annotations": annotations, "video_id": video_id})

    def evaluate(self):
        import json
        import torch.distributed as dist
        from .evaluation import _gather
        self._png.drain()
        if self._distributed:
            predictions = [p for part in _gather(self._predictions, True) for p in part]      # rank order, as comm.gather
            if dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
                return {}
        else:
            predictions = self._predictions
        if len(predictions) == 0:
            self._logger.warning("[VPSPredictionWriter] Did not receive valid predictions.")
            return {}
        if self._output_dir:
            with open(os.path.join(self._output_dir, "pred.json"), "w") as f:
                json.dump({"annotations": predictions}, f)
        return {}


class VSSPredictionWriter:
    """VSPW prediction files, as dvis_Plus/data_video/vss_eval.py writes them: <output_dir>/<video>/<frame>.png, uint8 dataset ids.

    Same constructor as the reference.  The prediction is cast to uint8 (value & 255), the ignore label becomes 255 and contiguous
    class c becomes the c-th KEY of `stuff_dataset_id_to_contiguous_id` (the reference builds its map from the keys); a class
    without one raises the reference's KeyError before the video's files are written.  The metadata's `ignore_label` and
    `stuff_dataset_id_to_contiguous_id`, or the keyword overrides of the same names.  evaluate() waits for the PNGs and returns {}."""

    def __init__(self, dataset_name, tasks=None, distributed=True, output_dir=None, *, use_fast_impl=True,
                 stuff_dataset_id_to_contiguous_id=None, ignore_label=None, device=None, encode_threads=MAX_ENCODE_THREADS):
        from .evaluation import _metadata
        meta = None
        if stuff_dataset_id_to_contiguous_id is None or ignore_label is None:
            meta = _metadata(dataset_name, "stuff_dataset_id_to_contiguous_id and ignore_label")
        ids = (stuff_dataset_id_to_contiguous_id if stuff_dataset_id_to_contiguous_id is not None
               else meta.stuff_dataset_id_to_contiguous_id)
        self.ignore_val = ignore_label if ignore_label is not None else meta.ignore_label
        self.contiguous_id_to_dataset_id = dict(enumerate(ids.keys()))
        lut = np.full(256, -1, np.int32)
        for c, d in self.contiguous_id_to_dataset_id.items():
            if c < 256:
                if not 0 <= int(d) <= 255:
                    raise ValueError(f"dataset id {d} of class {c} does not fit the uint8 PNG")
                lut[c] = int(d)
        if 0 <= int(self.ignore_val) <= 255:
            lut[int(self.ignore_val)] = 255
        self.lut = lut
        self._distributed, self._output_dir, self._device = distributed, output_dir, device
        self._png = _PngWriter(encode_threads)

    @property
    def host_bytes(self):
        """Bytes copied device -> host by process() so far (the painted maps and the unmapped-class counts)."""
        return self._png.host_bytes

    def reset(self):
        if self._output_dir is None:
            raise ValueError("VSSPredictionWriter needs an output_dir")
        self._png.drain()
        os.makedirs(self._output_dir, exist_ok=True)

    def process(self, inputs, outputs):
        from .evaluation import _device
        assert len(inputs) == 1, "More than one inputs are loaded for inference!"
        video_id = inputs[0]["video_id"]
        image_names = [inputs[0]["file_names"][idx] for idx in inputs[0]["frame_idx"]]
        sem = outputs["pred_masks"]
        if sem.dim() != 3 or len(image_names) > sem.shape[0]:
            raise ValueError(f"video {video_id}: pred_masks {tuple(sem.shape)} does not hold {len(image_names)} frames")
        sem = sem.to(_device(sem, self._device))
        out, bad = Fn.sem_paint(sem, torch.from_numpy(self.lut).to(sem.device))
        (out, bad), buf = self._png.to_host([out, bad])
        missing = np.flatnonzero(bad.numpy())
        if missing.size:
            self._png.submit([], buf)
            raise KeyError(int(missing[0]))
        out = out.numpy()
        vdir = os.path.join(self._output_dir, video_id)
        os.makedirs(vdir, exist_ok=True)
        self._png.submit([(os.path.join(vdir, _png_stem(nm) + ".png"), out[i]) for i, nm in enumerate(image_names)], buf)

    def evaluate(self):
        self._png.drain()
        return {}
