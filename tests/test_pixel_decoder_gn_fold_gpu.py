"""GPU: MSDeformAttnPixelDecoder.forward_features with the mask path's GroupNorms folded into its convolutions (default) against
DVIS_PD_GN_FOLD=0, the separate statistics / normalisation passes, on a 2-frame 96 x 160 input (stride-4 map 24 x 40 = 960
pixels = 30 wave slots per frame).

The encoder side does not pass through the changed code: out[0] and the multi-scale features must be the same bits.
mask_features is compared with an fp64 evaluation of the mask path's modules (lateral 1x1 -> GroupNorm -> + bilinear(top) ->
3x3 -> GroupNorm -> ReLU -> mask_features 1x1; `top` = the finest encoder map, identical in both runs).  The folded run's error may
exceed the separate run's OWN error only by what a 1-ulp difference of the two GroupNorms' (scale, shift) explains (the folded
statistics are the same fp64 sums in another order, tests/test_conv_gn_fold_gpu.py; everything else is the same arithmetic on the
same operands): per element of a normalised map 2^-23 (|x * scale| + |shift|), carried to the output through |W| of the
convolutions behind it and the factor |scale| of the second GroupNorm (first order)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _decoder():
    from dvis_plus_amd.pixel_decoder import MSDeformAttnPixelDecoder, r50_input_shape
    torch.manual_seed(3)
    pd = MSDeformAttnPixelDecoder(r50_input_shape(), transformer_dropout=0.0, transformer_nheads=8, transformer_dim_feedforward=1024,
                                  transformer_enc_layers=1, conv_dim=256, mask_dim=256, norm="GN",
                                  transformer_in_features=["res3", "res4", "res5"], common_stride=4).eval()
    with torch.no_grad():
        for m in pd.modules():                              # GroupNorm weights and biases that are not 1 and 0
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
    return pd.to(DEV)


class _Spy:
    """Counts the calls of C entry points (the ctypes functions are replaced on the library object, as bench.py's timers do)."""

    def __init__(self, lib, names):
        self.lib, self.names, self.calls, self.orig = lib, names, {n: 0 for n in names}, {}

    def __enter__(self):
        for n in self.names:
            self.orig[n] = getattr(self.lib, n)

            def counted(*args, _n=n):
                self.calls[_n] += 1
                return self.orig[_n](*args)
            setattr(self.lib, n, counted)
        return self

    def __exit__(self, *exc):
        for n in self.names:
            setattr(self.lib, n, self.orig[n])


def test_folded_mask_path_matches_the_separate_passes(monkeypatch):
    from dvis_plus_amd import functions as Fn, native
    pd = _decoder()
    g = torch.Generator().manual_seed(9)
    Hh, Ww = 96, 160
    feats = {k: (0.3 + torch.randn(2, c, Hh // s, Ww // s, generator=g)).to(DEV) for k, c, s in
             (("res2", 256, 4), ("res3", 512, 8), ("res4", 1024, 16), ("res5", 2048, 32))}
    names = ("dvis_scale_shift_act", "dvis_group_norm_affine", "dvis_group_norm_finalize")
    runs = {}
    with torch.no_grad():
        for fold in (True, False):
            monkeypatch.setattr(Fn, "PD_GN_FOLD", fold)
            with _Spy(native.lib(), names) as spy:
                mf, out0, ms = pd.forward_features(feats)
            Fn.X3_GUARD.check_now(torch.device(DEV))
            runs[fold] = (mf, out0, list(ms), dict(spy.calls))
    (mf1, o1, ms1, calls1), (mf0, o0, ms0, calls0) = runs[True], runs[False]
    # the C ABI: no in-place normalisation pass, statistics passes only for the three input projections
    assert calls1 == {"dvis_scale_shift_act": 0, "dvis_group_norm_affine": 3, "dvis_group_norm_finalize": 2}, calls1
    assert calls0 == {"dvis_scale_shift_act": 1, "dvis_group_norm_affine": 5, "dvis_group_norm_finalize": 0}, calls0
    assert torch.equal(o1, o0)
    assert len(ms1) == len(ms0) == 3 and all(torch.equal(a, b) for a, b in zip(ms1, ms0))

    # fp64 evaluation of the mask path's modules on the CPU
    with torch.no_grad():
        lat, oc, mfc = pd.lateral_convs[0], pd.output_convs[0], pd.mask_features
        d = lambda t: t.detach().double().cpu()
        x, top = d(feats["res2"]), d(ms1[2])
        l = F.conv2d(x, d(lat.weight))
        ln = F.group_norm(l, 32, d(lat.norm.weight), d(lat.norm.bias), lat.norm.eps)
        y = ln + F.interpolate(top, size=l.shape[-2:], mode="bilinear", align_corners=False)
        c = F.conv2d(y, d(oc.weight), None, 1, 1)
        cn = F.group_norm(c, 32, d(oc.norm.weight), d(oc.norm.bias), oc.norm.eps)
        ref = F.conv2d(cn.relu(), d(mfc.weight), d(mfc.bias))
        # what 1 ulp of (scale, shift) explains, first order: rel = 2^-23 on each term of x * scale + shift
        u = 2.0 ** -23
        cs = (cn - d(oc.norm.bias).view(1, -1, 1, 1)).abs() + d(oc.norm.bias).abs().view(1, -1, 1, 1)      # |c * scale| + ... >= |cn - beta| + |beta|
        a_out = F.conv2d(u * 2 * cs, d(mfc.weight).abs())
        ls = (ln - d(lat.norm.bias).view(1, -1, 1, 1)).abs() + d(lat.norm.bias).abs().view(1, -1, 1, 1)
        var = c.view(2, 32, -1).var(-1, unbiased=False)
        scale_c = (d(oc.norm.weight).view(1, 32, 8).abs() / (var.view(2, 32, 1) + oc.norm.eps).sqrt()).reshape(2, 256, 1, 1)
        a_lat = F.conv2d(F.conv2d(u * 2 * ls, d(oc.weight).abs(), None, 1, 1) * scale_c, d(mfc.weight).abs())
        allow = float((a_out + a_lat).max())
    e1 = float((mf1.double().cpu() - ref).abs().max())
    e0 = float((mf0.double().cpu() - ref).abs().max())
    print("mask_features max error vs fp64: folded %.3e separate %.3e allowance %.3e; bit-equal: %s" %
          (e1, e0, allow, torch.equal(mf1, mf0)))
    assert e0 < 1e-3                                         # (the separate run is itself fp32-grade: the comparison means something)
    assert e1 <= e0 + allow
