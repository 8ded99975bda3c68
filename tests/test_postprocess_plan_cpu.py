"""functions.postprocess_plan / dvis_postprocess_plan: how csrc/postprocess.hip cuts a call into workgroups and grid-stride sweeps
and which form of the semantic arg-max serves it, asked of the host function the launches themselves consult (no GPU: only sizes
are read).  The GPU file (test_postprocess_edges_gpu.py) asserts its cases' plans; this one pins where the boundaries are."""
import pytest

import postprocess_cases as PC


def plan(op, K, T, img, out, C=None):
    from dvis_plus_amd import functions as Fn
    return Fn.postprocess_plan(op, K, T, img, out, C)


@pytest.mark.parametrize("C,stride,K4", [(1, 32, 8), (32, 32, 8), (33, 64, 16), (64, 64, 16), (65, 96, 24), (96, 96, 24),
                                         (97, 128, 32), (128, 128, 32)])
def test_class_count_to_row_stride_to_K4(C, stride, K4):
    from dvis_plus_amd import functions as Fn
    assert Fn.vss_row_stride(C) == stride
    for Q in (5, 8):
        for img, out in (((24, 32), (24, 32)), ((37, 53), (30, 45))):
            p = plan("vss_argmax", Q, 2, img, out, C)
            assert (p.row_stride, p.K4, p.identity) == (stride, K4, img == out)
            if p.form == "generic":
                assert p.lds_bytes == 0


@pytest.mark.parametrize("Q,C,img,out,form,K4,identity,lds", [
    (124, 124, (24, 32), (24, 32), "mfma", 32, True, 124 * 132 * 4),      # the last MFMA size: 65472 bytes <= 64 KB
    (128, 124, (24, 32), (24, 32), "generic", 32, True, 0),               # Q % 4 == 0 but 67584 bytes: falls back
    (126, 124, (24, 32), (24, 32), "generic", 32, True, 0),               # Q % 4 != 0
    (100, 124, (23, 32), (24, 32), "generic", 32, False, 0),              # img != out (rows)
    (100, 124, (24, 31), (24, 32), "generic", 32, False, 0),              # img != out (columns)
    (100, 124, (24, 32), (24, 32), "mfma", 32, True, 100 * 132 * 4),
    (100, 97, (24, 32), (24, 32), "mfma", 32, True, 100 * 132 * 4),       # row stride 128 from C = 97
    (100, 96, (24, 32), (24, 32), "generic", 24, True, 0),                # row stride 96
    (4, 128, (24, 32), (24, 32), "mfma", 32, True, 4 * 132 * 4),
    (3, 128, (24, 32), (24, 32), "generic", 32, True, 0),
])
def test_when_the_mfma_form_applies(Q, C, img, out, form, K4, identity, lds):
    p = plan("vss_argmax", Q, 1, img, out, C)
    assert (p.form, p.K4, p.identity, p.lds_bytes) == (form, K4, identity, lds)


def test_mfma_form_exactly_when_stride_128_q_mod_4_same_size_and_q_le_124():
    for Q in list(range(1, 20)) + list(range(116, 135)):
        for C in (64, 96, 97, 128):
            for img in ((24, 32), (23, 32)):
                p = plan("vss_argmax", Q, 1, img, (24, 32), C)
                want = -(-C // 32) * 32 == 128 and Q % 4 == 0 and img == (24, 32) and Q <= 124
                assert (p.form == "mfma") == want, (Q, C, img, p)


# per-sweep capacity in work items, and the problem (K, T, out) that has n work items
ARGMAX_CAP = 256 * 16 * 256          # pixels
MFMA_CAP = 256 * 9 * 4               # 32-pixel wave chunks
RESIZE_CAP = 256 * 64 * 256          # floats / 4-pixel groups


@pytest.mark.parametrize("delta,sweeps", [(-1, 1), (0, 1), (1, 2)])
def test_sweeps_around_every_kernels_capacity(delta, sweeps):
    n = ARGMAX_CAP + delta
    for p in (plan("vps_argmax", 3, 1, (1, n), (1, n)), plan("vps_argmax", 3, 1, (7, 9), (1, n)),
              plan("vss_argmax", 5, 1, (1, n), (1, n), 8),             # generic: row stride 32
              plan("vss_argmax", 5, 1, (1, n), (1, n), 128),            # generic: Q % 4 != 0
              plan("vss_argmax", 8, 1, (2, n), (1, n), 128)):           # generic: img != out
        assert (p.workgroups, p.sweeps) == (min(-(-n // 256), 256 * 16), sweeps), p
        assert p.form in (None, "generic")
    # the MFMA form counts chunks of 32 pixels: one pixel past a full chunk is one more chunk
    chunks = MFMA_CAP + delta
    for npix in (32 * chunks, 32 * chunks - 31):
        p = plan("vss_argmax", 8, 1, (1, npix), (1, npix), 97)
        assert p.form == "mfma" and (p.workgroups, p.sweeps) == (min(-(-chunks // 4), 256 * 9), sweeps), p
    n = RESIZE_CAP + delta
    p = plan("resize2", 1, 1, (1, n), (1, n))
    assert (p.workgroups, p.sweeps) == (min(-(-n // 256), 256 * 64), sweeps), p
    for out in ((1, 4 * n), (1, 4 * n - 3)):                            # a group is 4 pixels of one row, the last may be partial
        p = plan("resize2_gt0", 1, 1, out, out)
        assert (p.workgroups, p.sweeps) == (min(-(-n // 256), 256 * 64), sweeps), p


def test_small_grids_and_many_sweeps():
    assert plan("vps_argmax", 5, 2, (37, 53), (30, 45))[:2] == (-(-2 * 30 * 45 // 256), 1)
    assert plan("vss_argmax", 8, 1, (24, 32), (24, 32), 128)[:2] == (-(-(24 * 32 // 32) // 4), 1)
    assert plan("resize2", 3, 2, (37, 53), (30, 45))[:2] == (-(-3 * 2 * 30 * 45 // 256), 1)
    assert plan("resize2_gt0", 3, 2, (37, 53), (30, 45))[:2] == (-(-3 * 2 * 30 * 12 // 256), 1)      # ceil(45 / 4) = 12 groups a row
    assert plan("vps_argmax", 20, 30, (720, 1280), (720, 1280))[:2] == (4096, -(-30 * 720 * 1280 // ARGMAX_CAP))
    assert plan("vss_argmax", 100, 30, (720, 1280), (720, 1280), 124)[:2] == (2304, -(-30 * 720 * 1280 // 32 // MFMA_CAP))
    # the gt0 groups do not straddle rows: out_w = 5 is two groups a row
    assert plan("resize2_gt0", 1, 1, (8, 8), (RESIZE_CAP // 2, 5)).sweeps == 1
    assert plan("resize2_gt0", 1, 1, (8, 8), (RESIZE_CAP // 2 + 1, 5)).sweeps == 2


def test_edge_cases_of_the_gpu_file_make_two_sweeps():
    """The large shapes of test_postprocess_edges_gpu.py (section e), pinned here so that a change of a cap shows on the CPU."""
    for name, (op, K, T, geom, C) in PC.SWEEP_CASES.items():
        p = plan(op, K, T, geom[2], geom[3], C)
        assert p.sweeps == 2, (name, p)
        assert p.form == {"vss_argmax-generic": "generic", "vss_argmax-mfma": "mfma"}.get(name), (name, p)


def test_nothing_to_launch():
    for op, C in (("vps_argmax", None), ("vss_argmax", 8), ("resize2", None), ("resize2_gt0", None)):
        p = plan(op, 3, 0, (24, 32), (24, 32), C)
        assert (p.workgroups, p.sweeps) == (0, 0)
    for op in ("resize2", "resize2_gt0"):
        assert plan(op, 0, 2, (24, 32), (24, 32))[:2] == (0, 0)


def test_plan_refuses_what_the_launch_refuses():
    assert plan("vps_argmax", 256, 1, (24, 32), (24, 32)).workgroups == 3
    with pytest.raises(RuntimeError, match=r"K must be 1\.\.256"):
        plan("vps_argmax", 257, 1, (24, 32), (24, 32))
    with pytest.raises(RuntimeError, match=r"K must be 1\.\.256"):
        plan("vps_argmax", 0, 1, (24, 32), (24, 32))
    with pytest.raises(RuntimeError, match=r"C must be 1\.\.128"):
        plan("vss_argmax", 8, 1, (24, 32), (24, 32), 129)
    with pytest.raises(RuntimeError, match="2\\^31 output pixels"):
        plan("vps_argmax", 3, 1, (8, 8), (1 << 16, 1 << 15))
    with pytest.raises(RuntimeError, match="class count of vss_argmax"):
        plan("vss_argmax", 8, 1, (24, 32), (24, 32))
    with pytest.raises(RuntimeError, match="class count of vss_argmax"):
        plan("resize2", 8, 1, (24, 32), (24, 32), 5)
    with pytest.raises(ValueError):
        plan("argmax", 8, 1, (24, 32), (24, 32))
