"""Inputs and torch-CPU references shared by the post-processing tests (test_postprocess_gpu.py, test_postprocess_edges_gpu.py,
test_postprocess_plan_cpu.py).  Nothing here touches the GPU: a case is built and its reference computed on the host, the GPU files
hand the same values to csrc/postprocess.hip.

The reference is always the sequence the reference implementation runs on CPU tensors: F.interpolate -> crop -> (sigmoid) ->
F.interpolate (`_cpu_sequence`), then arg-max / threshold / bincount in torch."""
import torch
import torch.nn.functional as F

# small geometries, hw -> first -> img -> out
S1 = ((6, 8), (24, 32), (24, 32), (24, 32))          # second stage is the identity, no crop
S2 = ((10, 14), (40, 56), (37, 53), (30, 45))        # both stages real, crop in x (scalar-exp tail columns), h + w <= 128 twice
GEN = ((12, 20), (48, 80), (45, 77), (90, 160))      # first stage small kernel (48 + 80 = 128), second generic

# the only large shapes: one launch each that needs a second grid-stride sweep.  name -> (op, K or Q, T, geometry, C)
SWEEP_CASES = {
    "vps_argmax": ("vps_argmax", 3, 2, ((46, 80), (184, 320), (180, 300), (720, 1200)), None),
    "vss_argmax-generic": ("vss_argmax", 5, 1, ((46, 80), (184, 320), (180, 300), (900, 1200)), 8),
    "vss_argmax-mfma": ("vss_argmax", 8, 1, ((120, 160), (480, 640), (480, 640), (480, 640)), 97),
    "resize2": ("resize2", 3, 2, ((46, 80), (184, 320), (180, 300), (720, 1200)), None),
    "resize2_gt0": ("resize2_gt0", 10, 2, ((46, 80), (184, 320), (180, 300), (720, 1200)), None),
}


def _logits(K, T, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, K, *hw, generator=g) * 3).permute(1, 0, 2, 3)      # (K,T,h,w) strided like mask_fn's output


def _cpu_sequence(logits, first, img, out, sigmoid):
    m = F.interpolate(logits.contiguous(), size=first, mode="bilinear", align_corners=False)[:, :, :img[0], :img[1]]
    if sigmoid:
        m = m.sigmoid()
    return F.interpolate(m, size=out, mode="bilinear", align_corners=False)


def stage_one(logits, first, img):
    """The values the sigmoid sees: the first resize, cropped."""
    return F.interpolate(logits.contiguous(), size=first, mode="bilinear", align_corners=False)[:, :, :img[0], :img[1]]


def tk_view(values):
    """(K, T, h, w) values as the (T, K)-permuted view `_logits` returns (what mask_fn hands over)."""
    return values.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)


def layouts(values, filler_seed=99):
    """The same (K, T, h, w) values in three layouts: the (T, K)-permuted view, contiguous, and every second candidate of a
    (2K, T, h, w) tensor starting one candidate in (the other candidates hold different values).  Built by `to` on the caller's
    device: [(name, function of a device -> tensor)]."""
    K = values.shape[0]

    def strided(dev):
        g = torch.Generator().manual_seed(filler_seed)
        big = (torch.randn(2 * K, *values.shape[1:], generator=g) * 3).to(dev)
        big[1::2] = values.to(dev)
        return big[1::2]
    return [("tk-permuted", lambda dev: tk_view(values).to(dev)),           # .to keeps the strides of a dense permuted tensor
            ("contiguous", lambda dev: values.contiguous().to(dev)),
            ("every-second", strided)]


def vps_reference(logits, scores, first, img, out):
    """ids (T, H, W) int64, conf bool, areas (3, K) int64 of the torch CPU sequence; torch.argmax returns the first maximum."""
    K = logits.shape[0]
    m = _cpu_sequence(logits, first, img, out, True)
    ids = (scores.view(-1, 1, 1, 1) * m).argmax(0)
    conf = m.gather(0, ids[None])[0] >= 0.5
    areas = torch.stack([torch.bincount(ids.flatten(), minlength=K), (m >= 0.5).flatten(1).sum(1),
                         torch.bincount(ids.flatten(), weights=conf.flatten().double(), minlength=K).long()])
    return ids, conf, areas, m


def vss_inputs(Q, C, T, hw):
    """The existing rule of test_vss_argmax_vs_torch_sequence: seed Q + C, logits randn * 3, cls = softmax(randn * 2)[:, :-1]."""
    g = torch.Generator().manual_seed(Q + C)
    logits = _logits(Q, T, hw, Q + C)
    cls = torch.softmax(torch.randn(Q, C + 1, generator=g) * 2, -1)[:, :-1]
    return logits, cls


def class_sums64(cls, m, band=None):
    """fp64 class sums (C, T, H, W) of probabilities m (Q, T, H, W); `band`: rows per einsum (bounds the fp64 copy of m)."""
    if band is None:
        return torch.einsum("qc,qthw->cthw", cls.double(), m.double())
    return torch.cat([torch.einsum("qc,qthw->cthw", cls.double(), m[:, :, y:y + band].double())
                      for y in range(0, m.shape[2], band)], 2)


def vss_reference(logits, cls, first, img, out, band=None):
    """(want, margin, tol, n_unsafe): the fp64 arg-max, its top-2 margin, the tolerance 2e-6 * sem.max() of the existing test and the
    number of pixels at which the REFERENCE alone is not decisive — the fp32 CPU arg-max differs from the fp64 one, or the margin is
    within the tolerance."""
    m = _cpu_sequence(logits, first, img, out, True)
    sem = class_sums64(cls, m, band)
    want = sem.max(0)[1]
    top2 = sem.topk(2, dim=0)[0] if sem.shape[0] > 1 else None
    margin = top2[0] - top2[1] if top2 is not None else torch.full_like(sem[0], float("inf"))
    tol = 2e-6 * float(sem.max())
    want32 = torch.einsum("qc,qthw->cthw", cls, m).max(0)[1]
    n_unsafe = int(((want32 != want) | (margin <= tol)).sum())
    return want, margin, tol, n_unsafe


def tie_cls(Q, C, lo, hi, seed):
    """Class scores whose columns lo and hi are the same vector in [0.5, 1) and every other column is below 0.01: the two class
    sums are the same fp32 operation sequence on the same operands, so they tie bit for bit, far above the rest."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.rand(Q, C, generator=g) * 0.01
    v = torch.rand(Q, generator=g) * 0.5 + 0.5
    cls[:, lo] = v
    cls[:, hi] = v
    return cls


def saturating_logits(K, T, hw, seed):
    """`_logits` with candidate k multiplied by 1, 6, 30, 1, ...: sigmoid arguments from the usual range to beyond both cut-offs of
    the exp (|x| > 104), through the range where the sigmoid is a denormal (about -88.7 < x < -87.3)."""
    factor = torch.tensor([1.0, 6.0, 30.0]).repeat((K + 2) // 3)[:K]
    return tk_view(_logits(K, T, hw, seed) * factor.view(-1, 1, 1, 1))
