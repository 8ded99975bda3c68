"""CPU: the test-time resize of decoded frames (functions.resize_frames_u8 on CPU tensors = cpu_ops over the coefficient tables the
kernel uses) byte-identical to Pillow's Image.resize(BILINEAR), detectron2's ResizeShortestEdge output size, and the wiring of
dvis_plus_amd.predictor.VideoPredictor (cfg keys, defaults, strict weight load, what the model is handed)."""
import numpy as np
import pytest
import torch
from PIL import Image

from dvis_plus_amd import cpu_ops
from dvis_plus_amd import functions as Fn
from dvis_plus_amd.config import get_default_cfg
from dvis_plus_amd.predictor import VideoPredictor, resize_shortest_edge_size


@pytest.mark.parametrize("hw_short_max, out", [
    ((720, 1280, 480, 1333), (480, 853)),
    ((1080, 1920, 480, 1333), (480, 853)),
    ((1280, 720, 480, 1333), (853, 480)),
    ((720, 1280, 720, 1333), (720, 1280)),
    ((360, 640, 720, 1333), (720, 1280)),
    ((481, 853, 480, 1333), (480, 851)),
    ((400, 2000, 480, 1333), (267, 1333)),
])
def test_resize_shortest_edge_size(hw_short_max, out):
    assert resize_shortest_edge_size(*hw_short_max) == out


def pil_resize(f, h, w):
    return np.array(Image.fromarray(f).resize((w, h), Image.BILINEAR))


def frame(H, W, kind, seed):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    cb = (((yy + xx + seed) % 2) * 255).astype(np.uint8)
    return np.stack([cb, 255 - cb, cb], -1)              # 0 / 255 checkerboards drive clip8 to both ends


# (H, W) -> (h, w): down-scales by 1.5 and 2.25, identity, up-scales, one axis only, odd sizes, 1-pixel-wide / -high frames
CASES = [
    ((144, 256), (96, 171)),        # 1.5x (720p -> 480p, scaled down)
    ((216, 384), (96, 171)),        # 2.25x (1080p -> 480p, scaled down)
    ((97, 171), (96, 170)),         # 481 x 853 -> 480 x 851 in shape
    ((45, 80), (45, 80)),           # identity
    ((36, 64), (72, 128)),          # 360 -> 720
    ((48, 64), (72, 96)),           # 480 -> 720
    ((50, 60), (50, 37)),           # width only
    ((50, 60), (23, 60)),           # height only
    ((37, 53), (29, 71)),           # odd, one axis up, one down
    ((40, 1), (25, 1)),             # 1 pixel wide
    ((1, 40), (1, 25)),             # 1 pixel high
    ((1, 1), (3, 5)),
    ((7, 1), (2, 3)),
]


@pytest.mark.parametrize("src, dst", CASES)
@pytest.mark.parametrize("kind", ["random", "checkerboard"])
def test_cpu_resize_equals_pillow(src, dst, kind):
    frames = np.stack([frame(*src, kind, s) for s in range(2)])
    out = Fn.resize_frames_u8(torch.from_numpy(frames), dst)
    assert out.dtype == torch.uint8 and out.shape == (2, 3, *dst)
    for t in range(2):
        assert torch.equal(out[t].permute(1, 2, 0), torch.from_numpy(pil_resize(frames[t], *dst)))


def test_720p_frame_equals_pillow():
    f = frame(720, 1280, "random", 7)
    out = Fn.resize_frames_u8(torch.from_numpy(f)[None], (480, 853))
    assert torch.equal(out[0].permute(1, 2, 0), torch.from_numpy(pil_resize(f, 480, 853)))


def test_channel_reversal():
    f = frame(30, 50, "random", 3)
    x = torch.from_numpy(f)[None]
    plain = Fn.resize_frames_u8(x, (20, 33))
    rev = Fn.resize_frames_u8(x, (20, 33), reverse_channels=True)
    assert torch.equal(rev, plain.flip(1))
    assert torch.equal(rev[0].permute(1, 2, 0), torch.from_numpy(pil_resize(np.ascontiguousarray(f[:, :, ::-1]), 20, 33)))


def test_tables():
    """Identity axis: [x, taps, 2^22, 0]; coefficients are Pillow's: non-negative, zero past the taps, summing to ~2^22."""
    t = Fn.resize_tables(10, 10)
    assert t.shape == (10, 5) and torch.equal(t[:, 0], torch.arange(10, dtype=torch.int32))
    assert torch.equal(t[:, 2:4], torch.tensor([[1 << 22, 0]] * 10, dtype=torch.int32))
    assert Fn.resize_tables(10, 10) is t                       # cached
    t = Fn.resize_tables(1920, 853)
    assert t.shape[1] == 2 + 7 and (t[:, 2:] >= 0).all()
    taps = t[:, 1].long()
    assert ((t[:, 2:].long().sum(1) - (1 << 22)).abs() <= 4).all()
    assert all(int(t[o, 2 + int(taps[o]):].abs().sum()) == 0 for o in range(0, 853, 50))
    x = torch.from_numpy(frame(12, 1920, "random", 1))[None]
    assert torch.equal(cpu_ops.resize_frames_u8(x, t, Fn.resize_tables(12, 12)), Fn.resize_frames_u8(x, (12, 853)))


@pytest.mark.parametrize("bad, msg", [
    (torch.zeros((1, 8, 8, 3), dtype=torch.float32), "uint8"),
    (torch.zeros((1, 8, 8, 4), dtype=torch.uint8), r"\(T, H, W, 3\)"),
    (torch.zeros((8, 8, 3), dtype=torch.uint8), r"\(T, H, W, 3\)"),
    (torch.zeros((0, 8, 8, 3), dtype=torch.uint8), "no pixels"),
    (torch.zeros((1, 8, 16, 3), dtype=torch.uint8)[:, :, ::2], "contiguous"),
    (torch.zeros((1, 505, 5, 3), dtype=torch.uint8), "100 x"),
])
def test_rejected_inputs(bad, msg):
    with pytest.raises(RuntimeError, match=msg):
        Fn.resize_frames_u8(bad, (4, 4))


class Recorder(torch.nn.Module):
    """Stands in for a model: keeps what it was called with."""

    def __init__(self):
        super().__init__()
        self.register_buffer("pixel_mean", torch.zeros(3, 1, 1))
        self.calls = []

    def forward(self, batched_inputs):
        self.calls.append(batched_inputs)
        return {"n": len(self.calls)}


@pytest.mark.parametrize("fmt", ["BGR", "RGB"])
def test_predictor_hands_the_model_resized_uint8_frames(fmt):
    m = Recorder()
    p = VideoPredictor(model=m, min_size_test=24, max_size_test=1333, input_format=fmt)
    frames = [frame(36, 64, "random", s)[:, ::-1] for s in range(3)]          # negative strides are fine
    assert p(frames) == {"n": 1}
    (inp,) = m.calls[0]
    assert inp["height"] == 36 and inp["width"] == 64 and inp["keep"] is False
    img = inp["image"]
    assert img.dtype == torch.uint8 and img.shape == (3, 3, 24, 43)
    for t, f in enumerate(frames):
        f = f[:, :, ::-1] if fmt == "RGB" else f
        ref = pil_resize(np.ascontiguousarray(f), 24, 43).astype("float32").transpose(2, 0, 1)    # the reference's recipe
        assert torch.equal(img[t].float(), torch.from_numpy(ref))
    p((torch.from_numpy(np.stack(frames)), True))
    assert m.calls[1][0]["keep"] is True and torch.equal(m.calls[1][0]["image"], img)


def test_predictor_rejects_empty_and_mixed_clips():
    p = VideoPredictor(model=Recorder(), min_size_test=24)
    with pytest.raises(RuntimeError, match="no frames"):
        p([])
    with pytest.raises(RuntimeError, match="no frames"):
        p(torch.zeros((0, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="one size"):
        p([frame(36, 64, "random", 0), frame(36, 62, "random", 0)])
    with pytest.raises(RuntimeError, match="uint8"):
        p([frame(36, 64, "random", 0).astype(np.float32)])
    with pytest.raises(RuntimeError, match="100 x"):
        p([frame(505, 5, "random", 0)])


def tiny_cfg(tmp_path):
    cfg = get_default_cfg()
    cfg.merge_from_list(["MODEL.SEM_SEG_HEAD.NUM_CLASSES", "5", "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", "1",
                         "MODEL.MASK_FORMER.DEC_LAYERS", "2", "MODEL.MASK_FORMER.NUM_OBJECT_QUERIES", "6",
                         "MODEL.MASK_FORMER.DIM_FEEDFORWARD", "64", "MODEL.TRACKER.DECODER_LAYERS", "1",
                         "MODEL.REFINER.DECODER_LAYERS", "1", "MODEL.DEVICE", "cpu",
                         "MODEL.WEIGHTS", str(tmp_path / "w.pth")])
    return cfg


def test_predictor_from_cfg(tmp_path):
    from dvis_plus_amd.config import build_model
    cfg = tiny_cfg(tmp_path)
    torch.manual_seed(0)
    src = build_model(cfg)
    sd = src.state_dict()
    torch.save({"model": sd, "iteration": 3}, cfg.MODEL.WEIGHTS)
    p = VideoPredictor(cfg)
    assert (p.min_size_test, p.max_size_test, p.input_format) == (800, 1333, "BGR")      # detectron2's defaults
    assert type(p.model).__name__ == "DVIS_Plus_offline" and not p.model.training
    assert all(torch.equal(v, sd[k]) for k, v in p.model.state_dict().items())
    assert "INPUT" in cfg and "MIN_SIZE_TEST" not in cfg.INPUT          # the caller's cfg is left alone

    cfg.merge_from_list(["INPUT.MIN_SIZE_TEST", "480", "INPUT.MAX_SIZE_TEST", "1000", "INPUT.FORMAT", "RGB"])
    torch.save(sd, cfg.MODEL.WEIGHTS)                                     # a bare state dict loads too
    p = VideoPredictor(cfg)
    assert (p.min_size_test, p.max_size_test, p.input_format) == (480, 1000, "RGB")

    torch.save({"model": {**sd, "extra.weight": torch.zeros(1)}}, cfg.MODEL.WEIGHTS)
    with pytest.raises(RuntimeError, match="extra.weight"):
        VideoPredictor(cfg)                                               # strict=True
    sd.pop(next(iter(sd)))
    torch.save(sd, cfg.MODEL.WEIGHTS)
    with pytest.raises(RuntimeError, match="Missing"):
        VideoPredictor(cfg)
