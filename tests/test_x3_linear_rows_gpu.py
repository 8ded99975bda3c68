"""GPU: dvis_x3_linear_rows / dvis_x3_linear_add_rows (csrc/gemm_x3.hip) — the split-f16 projections on one level's rows of an
(N, S, C) token tensor read where they lie (row r at (r / rows_per_batch) * batch_stride + (r % rows_per_batch) * ldx) against the
single-stride entries on the compaction of the same rows: the same summation order per row, so the same bits.

(N, S, C) = (3, 315, 256) with levels of 15, 60 and 240 rows: at 60 rows per frame the 32-row wave tiles straddle frames (rows
32 .. 63 of the call hold frame 0's last 28 rows and frame 1's first 4).  Also N = 1, a 920-row level of two frames (the 720p
pyramid's coarsest level: 920 is no multiple of 32 either), and operands the entries refuse."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _weights(n_out, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n_out, 256, generator=g) / 16).to(DEV), torch.randn(n_out, generator=g).to(DEV)


def _both_forms(y, lo, hi, n_out, seed):
    """(in place, on the compaction) for the plain form and the xadd form of rows [lo, hi) of every frame of y."""
    from dvis_plus_amd import functions as Fn
    W, b = _weights(n_out, seed)
    g = torch.Generator().manual_seed(seed + 1)
    pos = torch.randn(1, hi - lo, 256, generator=g).to(DEV)
    view = y[:, lo:hi]
    comp = view.contiguous()
    assert y.shape[0] == 1 or Fn.x3_rows_in_place(view, n_out)
    assert not Fn.x3_rows_in_place(comp, n_out)
    plain = (Fn.x3_linear(view, W, b), Fn.x3_linear(comp, W, b))
    add = (Fn.x3_linear(view, W, b, xadd=pos), Fn.x3_linear(comp, W, b, xadd=pos))
    Fn.X3_GUARD.check_now(torch.device(DEV))
    return plain, add, (W, b, pos)


@pytest.mark.parametrize("lo,hi", [(15, 75), (0, 15), (75, 315)])
@pytest.mark.parametrize("n_out", [256, 768])
def test_a_levels_rows_in_place_give_the_compactions_bits(lo, hi, n_out):
    g = torch.Generator().manual_seed(hi)
    y = torch.randn(3, 315, 256, generator=g).to(DEV)
    plain, add, (W, b, pos) = _both_forms(y, lo, hi, n_out, seed=n_out + lo)
    assert torch.equal(*plain) and torch.equal(*add)
    assert not torch.equal(plain[0], add[0]) and bool(torch.isfinite(add[0]).all())      # (xadd took part)


def test_one_frame_and_a_920_row_level_of_two():
    from dvis_plus_amd import functions as Fn, native
    g = torch.Generator().manual_seed(920)
    y1 = torch.randn(1, 315, 256, generator=g).to(DEV)
    plain, add, (W, b, pos) = _both_forms(y1, 15, 75, 768, seed=5)
    assert torch.equal(*plain) and torch.equal(*add)
    # one frame through the rows entry itself (a (1, hw, C) slice is contiguous: x3_linear takes the single-stride entry for it)
    buf, wexp = Fn.x3_pack(W)
    out = torch.empty(1, 60, 768, device=DEV)
    view = y1[:, 15:75]
    native.check(native.lib().dvis_x3_linear_rows(
        ctypes.c_void_p(view.data_ptr()), 256, 60, 315 * 256, 60, 256, ctypes.c_void_p(buf.data_ptr()), 768, Fn.X3_XEXP, wexp,
        ctypes.c_void_p(b.data_ptr()), 0, ctypes.c_void_p(out.data_ptr()), 768, native.stream_ptr(torch.device(DEV))), "dvis_x3_linear_rows")
    assert torch.equal(out, plain[1])
    y2 = torch.randn(2, 920 + 3680, 256, generator=g).to(DEV)
    plain, add, _ = _both_forms(y2, 0, 920, 768, seed=6)
    assert torch.equal(*plain) and torch.equal(*add)
    plain, add, _ = _both_forms(y2, 920, 920 + 3680, 256, seed=7)
    assert torch.equal(*plain) and torch.equal(*add)


def test_refused_operands_raise_by_name():
    from dvis_plus_amd import functions as Fn, native
    lib = native.lib()
    W, b = _weights(768, 1)
    buf, wexp = Fn.x3_pack(W)
    y = torch.zeros(2, 64 * 256 + 8, device=DEV)               # frames 64 rows + 8 floats apart
    out = torch.empty(2, 60, 768, device=DEV)
    st = native.stream_ptr(torch.device(DEV))

    def call(batch_stride, rows=60, M=120, n_out=768):
        return lib.dvis_x3_linear_rows(ctypes.c_void_p(y.data_ptr()), 256, rows, batch_stride, M, 256, ctypes.c_void_p(buf.data_ptr()),
                                       n_out, Fn.X3_XEXP, wexp, ctypes.c_void_p(b.data_ptr()), 0, ctypes.c_void_p(out.data_ptr()), n_out, st)
    native.check(call(64 * 256 + 8), "dvis_x3_linear_rows")           # a multiple of 4 floats: served
    for bad in (64 * 256 + 6, 64 * 256 + 1, 59 * 256):               # misaligned; frames that overlap
        with pytest.raises(RuntimeError, match="dvis_x3_linear_rows: batch_stride"):
            native.check(call(bad), "dvis_x3_linear_rows")
    with pytest.raises(RuntimeError, match="whole number of batches"):
        native.check(call(64 * 256 + 8, M=100), "dvis_x3_linear_rows")
    # a view x3_linear does not read in place is compacted, not refused
    view = y[:, :64 * 256 + 4].view(2, -1)[:, 2:2 + 60 * 256].view(2, 60, 256)      # batch stride % 4 == 0, base 8 bytes off 16
    assert not Fn.x3_rows_in_place(view, 768)
    assert torch.equal(Fn.x3_linear(view, W, b), Fn.x3_linear(view.contiguous(), W, b))
