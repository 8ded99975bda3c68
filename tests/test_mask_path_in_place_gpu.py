"""GPU: the encoder memory read in place behind the pixel decoder's encoder — the top-down kernel takes the finest level token-major
(dvis_upsample_add_image_tokens, no dvis_tokens_to_nchw) and the masked-attention decoder's K / V projections take each level's rows
where they lie (dvis_x3_linear_rows / _add_rows, no compaction) — against the same modules with both paths switched off
(the first kernel form on a transposed map; projections on compacted rows).  Data movement only: every output is the same bits.

MSDeformAttnPixelDecoder.forward_features + MultiScaleMaskedTransformerDecoder._run_layers on the 2-frame 96 x 160 input of
tests/test_pixel_decoder_gn_fold_gpu.py."""
import pytest
import torch

from test_pixel_decoder_gn_fold_gpu import _Spy, _decoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_in_place_reads_change_no_bit(monkeypatch):
    from dvis_plus_amd import functions as Fn, native
    from dvis_plus_amd.transformer_decoder import MultiScaleMaskedTransformerDecoder
    pd = _decoder()
    torch.manual_seed(4)
    dec = MultiScaleMaskedTransformerDecoder(256, True, num_classes=7, hidden_dim=256, num_queries=10, nheads=8, dim_feedforward=512,
                                             dec_layers=6, pre_norm=False, mask_dim=256, enforce_input_project=False).eval().to(DEV)
    g = torch.Generator().manual_seed(9)
    Hh, Ww = 96, 160
    feats = {k: (0.3 + torch.randn(2, c, Hh // s, Ww // s, generator=g)).to(DEV) for k, c, s in
             (("res2", 256, 4), ("res3", 512, 8), ("res4", 1024, 16), ("res5", 2048, 32))}
    lib = native.lib()
    names = ("dvis_tokens_to_nchw", "dvis_upsample_add_image_tokens", "dvis_upsample_add_image", "dvis_x3_linear_rows",
             "dvis_x3_linear_add_rows")
    runs = {}
    with torch.no_grad():
        for on in (True, False):
            monkeypatch.setattr(Fn, "X3_LINEAR_ROWS", on)
            prev = lib.dvis_upsample_add_image_set_v2(int(on))
            try:
                with _Spy(lib, names) as spy:
                    mf, out0, ms = pd.forward_features(feats)
                    output = dec._run_layers(ms, mf)
                Fn.X3_GUARD.check_now(torch.device(DEV))
            finally:
                lib.dvis_upsample_add_image_set_v2(prev)
            runs[on] = (mf, out0, list(ms), output, dict(spy.calls))
    (mf1, o1, ms1, d1, calls1), (mf0, o0, ms0, d0, calls0) = runs[True], runs[False]
    # the default run: no map transpose, the finest level read as tokens, all three levels projected in place
    assert calls1 == {"dvis_tokens_to_nchw": 0, "dvis_upsample_add_image_tokens": 1, "dvis_upsample_add_image": 0,
                      "dvis_x3_linear_rows": 3, "dvis_x3_linear_add_rows": 3}, calls1
    assert calls0 == {"dvis_tokens_to_nchw": 1, "dvis_upsample_add_image_tokens": 0, "dvis_upsample_add_image": 1,
                      "dvis_x3_linear_rows": 0, "dvis_x3_linear_add_rows": 0}, calls0
    assert torch.equal(mf1, mf0)
    assert torch.equal(o1, o0)
    assert len(ms1) == len(ms0) == 3 and all(torch.equal(a, b) for a, b in zip(ms1, ms0))
    assert torch.equal(d1, d0) and bool(torch.isfinite(d1).all())
