"""GPU: the prediction-file kernels (csrc/pred_write.hip) equal their CPU formulations exactly, and the VIPSeg / VSPW writers fed
device outputs write the reference's files (fixture g13) while copying only the painted maps and the stats table to the host."""
import os

import numpy as np
import pytest
import torch

from dvis_plus_amd import cpu_ops
from dvis_plus_amd import functions as Fn
import test_pred_writers_cpu as C
from test_pred_writers_cpu import g13  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def blocky_ids(T, H, W, lo, hi, cell, seed):
    """(T, H, W) int32 map of cell x cell blocks with ids in [lo, hi) that drift over the frames (segment-like runs)."""
    g = torch.Generator().manual_seed(seed)
    ch, cw = (H + cell - 1) // cell + 1, (W + cell - 1) // cell + 1
    cells = torch.randint(lo, hi, (T, ch, cw), generator=g, dtype=torch.int32)
    return cells.repeat_interleave(cell, 1).repeat_interleave(cell, 2)[:, :H, :W].contiguous()


def check_kernels(pan, n, nlut, seed):
    g = torch.Generator().manual_seed(seed)
    d = pan.to(DEV)
    stats, bad = Fn.pan_segment_stats(d, n)
    ref, ref_bad = cpu_ops.pan_segment_stats(pan, n)
    assert torch.equal(stats.cpu(), ref) and int(bad.item()) == ref_bad
    lut = torch.randint(0, 1 << 24, (nlut,), generator=g, dtype=torch.int32)
    assert torch.equal(Fn.pan_paint_rgb(d, lut.to(DEV)).cpu(), cpu_ops.pan_paint_rgb(pan, lut))
    slut = torch.randint(-1, 256, (256,), generator=g, dtype=torch.int32)
    out, sbad = Fn.sem_paint(d, slut.to(DEV))
    ref_out, ref_sbad = cpu_ops.sem_paint(pan, slut)
    assert torch.equal(out.cpu(), ref_out) and torch.equal(sbad.cpu(), ref_sbad)
    return ref


def test_kernels_on_a_720p_clip_lds_path():
    """30 frames of 720p, ~100 segments plus ids outside 0..n: the LDS stats table and the LDS colour table."""
    pan = blocky_ids(30, 720, 1280, -3, 104, 48, seed=1)
    ref = check_kernels(pan, 100, 101, seed=2)
    assert int(ref[0, :, 0].gt(0).sum()) >= 90


def test_kernels_with_more_ids_than_the_lds_tables_hold():
    """5000 ids: the stats table (3276 entries in 64 KB) and the colour table (4096 in LDS) take the global-memory paths."""
    pan = blocky_ids(4, 200, 300, -2, 5010, 3, seed=3)
    check_kernels(pan, 5000, 5001, seed=4)


@pytest.mark.parametrize("W", [1, 15, 17, 1281])
def test_widths_with_a_byte_tail(W):
    for T, H in [(1, 1), (3, 7), (2, 33)]:
        check_kernels(blocky_ids(T, H, W, -1, 12, 2, seed=W + T * H), 10, 9, seed=W)


def test_misaligned_views_are_painted_like_contiguous_maps():
    base = blocky_ids(1, 1, 3 * 5 * 7 + 1, 0, 6, 2, seed=9).view(-1)
    pan = base[1:].view(3, 5, 7)                                  # 4-byte offset: the wrappers realign
    lut = torch.arange(1, 7, dtype=torch.int32) * 0x010203
    assert torch.equal(Fn.pan_paint_rgb(base.to(DEV)[1:].view(3, 5, 7), lut.to(DEV)).cpu(), cpu_ops.pan_paint_rgb(pan, lut))


def test_vps_files_from_device_outputs(g13, tmp_path):
    C.write_vps(g13, str(tmp_path), device=DEV)
    C.check_vps_tree(g13, str(tmp_path))


def test_vss_files_from_device_outputs(g13, tmp_path):
    C.write_vss(g13, str(tmp_path), device=DEV)
    C.check_vss_tree(g13, str(tmp_path))


def test_unmapped_vss_class_raises_key_error_on_device(g13, tmp_path):
    w = C.vss_writer(g13, str(tmp_path), device=DEV)
    w.reset()
    k = next(i for i, v in enumerate(C.meta(g13)["vss"]) if "key_error" in v)
    with pytest.raises(KeyError) as e:
        w.process(*C.vss_inputs(g13, k, DEV))
    assert e.value.args[0] == C.meta(g13)["vss"][k]["key_error"]


def test_vps_copies_only_the_painted_map_and_the_stats(g13, tmp_path):
    w = C.vps_writer(g13, str(tmp_path), device=DEV)
    w.reset()
    want = 0
    for k in range(len(C.meta(g13)["vps"])):
        inputs, outputs = C.vps_inputs(g13, k, DEV)
        pan = outputs["pred_masks"]
        n = max(s["id"] for s in outputs["segments_infos"])
        np.random.seed(C.meta(g13)["seed"] + k)
        w.process(inputs, outputs)
        assert outputs["pred_masks"] is pan and pan.is_cuda
        want += pan.numel() * 3 + pan.shape[0] * (n + 1) * 5 * 8
        assert w.host_bytes == want
    w.evaluate()
    C.check_vps_tree(g13, str(tmp_path))


def test_reference_format_outputs_go_to_the_device(g13, tmp_path):
    """to_reference_format's CPU maps are moved to the device (device=None) and give the same files."""
    w = C.vps_writer(g13, str(tmp_path), device=None)
    w.reset()
    for k in range(len(C.meta(g13)["vps"])):
        np.random.seed(C.meta(g13)["seed"] + k)
        w.process(*C.vps_inputs(g13, k))
    w.evaluate()
    assert w.host_bytes > 0
    C.check_vps_tree(g13, str(tmp_path))


def test_round_trip_on_device(tmp_path, capsys):
    from conftest import GOLDEN
    C.roundtrip(np.load(os.path.join(GOLDEN, "g11_video_metrics.npz")), str(tmp_path), "cuda")
