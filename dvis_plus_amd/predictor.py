"""Video predictor: decoded uint8 frames at their own resolution in, the model's outputs out — the reference's "run a video" API
(demo_video/predictor.py:205-252, ``VideoPredictor``, also behind demo_long_video.py) with the test-time resize on the device.

The reference flips BGR to RGB when ``INPUT.FORMAT == "RGB"``, resizes every frame on one host thread with detectron2's
``ResizeShortestEdge([MIN_SIZE_TEST, MIN_SIZE_TEST], MAX_SIZE_TEST)`` (Pillow BILINEAR on uint8), then hands the model float32
CHW frames.  Here the clip is copied once into a recycled pinned buffer, goes to the device in one copy and is resized there by
csrc/frame_resize.hip (``functions.resize_frames_u8``), byte-identical to Pillow, with the channel flip folded into the write.
The model gets the uint8 (T, 3, h, w) clip: its preprocess converts uint8 exactly, so the outputs are those of the reference
recipe's float32 frames.
"""
import copy

import numpy as np
import torch

from . import functions as Fn

_DEFAULT_MIN_SIZE_TEST = 800        # detectron2's defaults (config/defaults.py: INPUT.MIN_SIZE_TEST, MAX_SIZE_TEST, FORMAT)
_DEFAULT_MAX_SIZE_TEST = 1333
_DEFAULT_FORMAT = "BGR"


def resize_shortest_edge_size(h, w, short, max_size):
    """(newh, neww) of detectron2's ResizeShortestEdge.get_output_shape: the short side to `short`, the long side capped at
    `max_size`, rounded half up.  short == 0 leaves the size unchanged (ResizeShortestEdge's NoOpTransform)."""
    h, w = int(h), int(w)
    if short == 0:
        return h, w
    scale = short * 1.0 / min(h, w)
    if h < w:
        newh, neww = short, scale * w
    else:
        newh, neww = scale * h, short
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh = newh * scale
        neww = neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def _cfg_get(cfg, path, default):
    node = cfg
    for key in path.split("."):
        try:
            node = node[key]
        except (KeyError, TypeError):
            return default
    return node


class VideoPredictor:
    """``VideoPredictor(cfg)``: the model of ``config.build_model(cfg)``, weights from ``torch.load(cfg.MODEL.WEIGHTS)`` (the
    ``"model"`` entry when there is one) loaded strictly, sizes and channel order from ``INPUT.MIN_SIZE_TEST`` /
    ``INPUT.MAX_SIZE_TEST`` / ``INPUT.FORMAT`` (detectron2's defaults 800 / 1333 / "BGR" when absent), on ``MODEL.DEVICE`` (default
    "cuda").  ``VideoPredictor(model=m, min_size_test=..., max_size_test=..., input_format=...)`` wraps a built model in place.

    ``predictor(frames)`` / ``predictor((frames, keep))``: frames = a list of (H, W, 3) uint8 BGR numpy arrays (any strides) or a
    (T, H, W, 3) uint8 tensor (host or device), all of one size.  Returns what the model returns for
    ``[{"image": (T, 3, h, w) uint8, "height": H, "width": W, "keep": keep}]``."""

    def __init__(self, cfg=None, *, model=None, min_size_test=_DEFAULT_MIN_SIZE_TEST, max_size_test=_DEFAULT_MAX_SIZE_TEST,
                 input_format=_DEFAULT_FORMAT):
        if (cfg is None) == (model is None):
            raise TypeError("VideoPredictor takes a cfg or a model=, not both")
        if cfg is not None:
            from .config import build_model
            self.cfg = copy.deepcopy(cfg)
            model = build_model(self.cfg).to(_cfg_get(cfg, "MODEL.DEVICE", "cuda"))
            model.eval()
            weight = torch.load(cfg.MODEL.WEIGHTS, map_location="cpu")
            if "model" in weight.keys():
                weight = weight["model"]
            model.load_state_dict(weight, strict=True)
            min_size_test = _cfg_get(cfg, "INPUT.MIN_SIZE_TEST", _DEFAULT_MIN_SIZE_TEST)
            max_size_test = _cfg_get(cfg, "INPUT.MAX_SIZE_TEST", _DEFAULT_MAX_SIZE_TEST)
            input_format = _cfg_get(cfg, "INPUT.FORMAT", _DEFAULT_FORMAT)
        self.model = model
        self.min_size_test, self.max_size_test = int(min_size_test), int(max_size_test)
        self.input_format = input_format
        assert self.input_format in ["RGB", "BGR"], self.input_format
        self._pinned = None          # recycled host staging buffer (flat uint8, pinned)
        self._pinned_free = None     # event recorded after the last copy out of it

    @property
    def device(self):
        p = getattr(self.model, "pixel_mean", None)
        return p.device if torch.is_tensor(p) else next(self.model.parameters()).device

    def _host_buffer(self, nbytes):
        """A pinned (nbytes,) uint8 view, free to overwrite: the previous clip's copy out of it has finished."""
        if self._pinned_free is not None:
            self._pinned_free.synchronize()
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)
        return self._pinned[:nbytes]

    def _upload(self, frames):
        """(T, H, W, 3) contiguous uint8 clip on the model's device."""
        dev = self.device
        if torch.is_tensor(frames):
            if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
                raise RuntimeError(f"VideoPredictor: a tensor clip must be (T, H, W, 3) uint8, got {tuple(frames.shape)} "
                                   f"{frames.dtype}")
            if frames.shape[0] == 0:
                raise RuntimeError("VideoPredictor: the clip has no frames")
            if frames.device == dev or dev.type != "cuda":
                return frames.to(dev).contiguous()
            shape = tuple(frames.shape)
            host = self._host_buffer(frames.numel()).view(shape)
            host.copy_(frames)
        else:
            frames = list(frames)
            if not frames:
                raise RuntimeError("VideoPredictor: the clip has no frames")
            for f in frames:
                if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                    raise RuntimeError("VideoPredictor: frames must be (H, W, 3) uint8 numpy arrays, got "
                                       f"{getattr(f, 'shape', None)} {getattr(f, 'dtype', type(f).__name__)}")
            if len({f.shape for f in frames}) != 1:
                raise RuntimeError(f"VideoPredictor: all frames of a clip must have one size, got {sorted({f.shape for f in frames})}")
            shape = (len(frames), *frames[0].shape)
            if dev.type != "cuda":
                return torch.from_numpy(np.stack(frames)).to(dev)
            host = self._host_buffer(int(np.prod(shape))).view(shape)
            dst = host.numpy()
            for t, f in enumerate(frames):
                np.copyto(dst[t], f)
        clip = torch.empty(shape, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            clip.copy_(host, non_blocking=True)
            if self._pinned_free is None:
                self._pinned_free = torch.cuda.Event()
            self._pinned_free.record()
        return clip

    def __call__(self, frames):
        if isinstance(frames, tuple):
            frames, keep = frames
        else:
            keep = False
        with torch.no_grad():
            clip = self._upload(frames)
            _, height, width, _ = clip.shape
            size = resize_shortest_edge_size(height, width, self.min_size_test, self.max_size_test)
            images = Fn.resize_frames_u8(clip, size, reverse_channels=self.input_format == "RGB")
            inputs = {"image": images, "height": int(height), "width": int(width), "keep": keep}
            return self.model([inputs])
