"""GPU: the frame resize kernel (csrc/frame_resize.hip) byte-identical to Pillow's Image.resize(BILINEAR) and to the CPU formulation,
and VideoPredictor end to end: its outputs equal those of the reference's recipe (Pillow-resized float32 CHW frames handed to the
same model)."""
import copy

import numpy as np
import pytest
import torch

from dvis_plus_amd import cpu_ops
from dvis_plus_amd import functions as Fn
from dvis_plus_amd.config import build_model, get_default_cfg
from dvis_plus_amd.predictor import VideoPredictor, resize_shortest_edge_size
from test_ingest_cpu import CASES, frame, pil_resize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def check_clip(frames, dst, reverse=False, every=1):
    """frames (T, H, W, 3) uint8 numpy: the kernel's output against Pillow for every `every`-th frame."""
    out = Fn.resize_frames_u8(torch.from_numpy(frames).to(DEV), dst, reverse_channels=reverse).cpu()
    assert out.shape == (len(frames), 3, *dst)
    for t in range(0, len(frames), every):
        f = np.ascontiguousarray(frames[t][:, :, ::-1]) if reverse else frames[t]
        assert torch.equal(out[t].permute(1, 2, 0), torch.from_numpy(pil_resize(f, *dst))), f"frame {t}"
    return out


@pytest.mark.parametrize("src, dst", CASES)
@pytest.mark.parametrize("kind", ["random", "checkerboard"])
def test_kernel_equals_pillow_and_cpu(src, dst, kind):
    frames = np.stack([frame(*src, kind, s) for s in range(3)])
    out = check_clip(frames, dst)
    assert torch.equal(out, Fn.resize_frames_u8(torch.from_numpy(frames), dst))
    rev = check_clip(frames, dst, reverse=True)
    assert torch.equal(rev, out.flip(1))


@pytest.mark.parametrize("src", [(720, 1280), (1080, 1920)])
def test_clip_of_36_frames_to_480p(src):
    g = torch.Generator().manual_seed(src[0])
    frames = torch.randint(0, 256, (36, *src, 3), generator=g, dtype=torch.uint8)
    frames[::5, ::7] = 255                                   # saturated rows in some frames
    dst = resize_shortest_edge_size(*src, 480, 1333)
    out = check_clip(frames.numpy(), dst)
    d = frames.to(DEV)
    assert all(torch.equal(Fn.resize_frames_u8(d, dst).cpu(), out) for _ in range(3))          # run-to-run identical
    assert torch.equal(cpu_ops.resize_frames_u8(frames[:1], Fn.resize_tables(src[1], dst[1]), Fn.resize_tables(src[0], dst[0])),
                       out[:1])


def test_4k_frame():
    f = frame(2160, 3840, "random", 11)
    check_clip(f[None], (480, 853))


def test_misaligned_and_odd_strided_inputs():
    """A frame view that does not start on a 16-byte boundary, odd sizes throughout."""
    base = torch.from_numpy(np.stack([frame(61, 97, "random", s) for s in range(3)])).to(DEV)
    flat = torch.empty(base.numel() + 5, dtype=torch.uint8, device=DEV)
    view = flat[5:].view(base.shape)
    view.copy_(base)
    assert view.data_ptr() % 16 != 0
    assert torch.equal(Fn.resize_frames_u8(view, (41, 65)), Fn.resize_frames_u8(base, (41, 65)))
    check_clip(base.cpu().numpy(), (41, 65))


# ---- VideoPredictor end to end on small random-init models -------------------------------------------------------------------
H, W, MIN = 240, 480, 128            # -> 128 x 256 frames for the model


def small_model(arch, task, fmt="BGR"):
    cfg = get_default_cfg()
    cfg.merge_from_list(["MODEL.META_ARCHITECTURE", arch, "MODEL.SEM_SEG_HEAD.NUM_CLASSES", "7",
                         "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", "1", "MODEL.MASK_FORMER.DEC_LAYERS", "3",
                         "MODEL.MASK_FORMER.NUM_OBJECT_QUERIES", "10", "MODEL.MASK_FORMER.TEST.TASK", task,
                         "MODEL.MASK_FORMER.TEST.MAX_NUM", "5", "MODEL.TRACKER.DECODER_LAYERS", "1",
                         "MODEL.REFINER.DECODER_LAYERS", "1", "INPUT.MIN_SIZE_TEST", str(MIN), "INPUT.FORMAT", fmt])
    if arch == "MinVIS":
        cfg.MODEL.MASK_FORMER.TRANSFORMER_DECODER_NAME = "VideoMultiScaleMaskedTransformerDecoder_minvis"
    torch.manual_seed(0)
    return cfg, build_model(cfg, n_things=4).to(DEV)


def reference_recipe(model, frames, fmt, keep=False):
    """demo_video/predictor.py:239-250: flip for "RGB", Pillow resize, astype(float32), transpose, then the model."""
    size = resize_shortest_edge_size(H, W, MIN, 1333)
    imgs = []
    for f in frames:
        f = np.ascontiguousarray(f[:, :, ::-1]) if fmt == "RGB" else f
        imgs.append(torch.as_tensor(pil_resize(f, *size).astype("float32").transpose(2, 0, 1)))
    with torch.no_grad():
        return model([{"image": imgs, "height": H, "width": W, "keep": keep}])


def assert_same(a, b, where="out"):
    assert type(a) is type(b), where
    if isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b), where
    elif torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), where
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            assert_same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same(x, y, f"{where}[{i}]")
    else:
        assert a == b, where


def clip(T, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H // 8, W // 8, 3), dtype=np.uint8)
    # blocky content with a moving bright square, so the models see structure that persists over the frames
    out = []
    for t in range(T):
        f = np.repeat(np.repeat(base, 8, 0), 8, 1).copy()
        f[40 + 5 * t:120 + 5 * t, 60 + 9 * t:180 + 9 * t] = (250, 30, 200)
        out.append(f)
    return out


@pytest.mark.parametrize("arch, task, fmt, as_tensor", [
    ("DVIS_Plus_offline", "vps", "BGR", False),
    ("DVIS_Plus_offline", "vps", "RGB", True),
    ("MinVIS", "vis", "RGB", False),
    ("MinVIS", "vis", "BGR", True),
])
def test_predictor_equals_reference_recipe(arch, task, fmt, as_tensor):
    cfg, model = small_model(arch, task, fmt)
    ref_model = copy.deepcopy(model)
    frames = clip(4, seed=len(arch))
    p = VideoPredictor(model=model, min_size_test=cfg.INPUT.MIN_SIZE_TEST, input_format=fmt)
    x = torch.from_numpy(np.stack(frames)) if as_tensor else [f[:, ::-1][:, ::-1] for f in frames]
    out = p(x)
    assert_same(out, reference_recipe(ref_model, frames, fmt))


def test_online_predictor_over_two_windows_with_keep():
    cfg, model = small_model("DVIS_Plus_online", "vps")
    ref_model = copy.deepcopy(model)
    frames = clip(6, seed=3)
    p = VideoPredictor(model=model, min_size_test=MIN)
    outs = [p((frames[:3], False)), p((torch.from_numpy(np.stack(frames[3:])).to(DEV), True))]
    refs = [reference_recipe(ref_model, frames[:3], "BGR"), reference_recipe(ref_model, frames[3:], "BGR", keep=True)]
    for o, r in zip(outs, refs):
        assert_same(o, r)
