"""The open-vocabulary (FC-CLIP) classification kernels on the GPU — csrc/mask_pool.hip, csrc/ov_class_logits.hip — against the fp64
CPU run at the project's 4 x rule (`check_4x`: the kernel may be 4 x as far from the fp64 CPU run as the fp32 CPU run is), their
bit-level properties, and the `_OV` decoders against golden g22 (the reference's own module)."""
import math

import pytest
import torch

import ov_heads_cases as C
from dvis_plus_amd import cpu_ops, functions as Fn
from vit_adapter_train_cases import check_4x

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(rtol=1e-3, atol=1e-3)         # the project's parity bar (tests/test_golden_gpu.py)


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _pool_case(B, Q, C, H, W, seed=0):
    return _rand(B, C, H, W, seed=seed), _rand(B, Q, H, W, seed=seed + 1)


def _check_pool(x, logits, what):
    """Fn.mask_pool on the GPU against the fp64 CPU run (4 x rule on the sums, counts exactly); -> the GPU results."""
    total, count = Fn.mask_pool(x.to(DEV), logits.to(DEV))
    s32, c32 = cpu_ops.mask_pool(x, logits)
    s64, c64 = cpu_ops.mask_pool(x.double(), logits.double())
    assert count.dtype == torch.int32 and torch.equal(count.cpu(), c64) and torch.equal(c32, c64)
    check_4x({"sum": total}, {"sum": s32}, {"sum": s64}, what + " ")
    return total, count


PLAN = Fn.mask_pool_plan(1, 5, 8, 1, 1)
THREE_SLABS = (1, 2 * PLAN.slab + 37)                                        # H x W: three slabs, the last one 37 pixels


@pytest.mark.parametrize("B,Q,C,H,W", [(1, 3, 4, 5, 7),                       # unaligned rows, everything a tail
                                       (2, 17, 20, 1, 67),                    # a second query tile of one row, C not a multiple of 16
                                       (1, 5, 8, *THREE_SLABS),               # >= 3 slabs with a partial last one (from the plan)
                                       (2, 100, 256, 48, 80),
                                       (1, 100, 1536, 6, 10)])                # channel chunks
def test_mask_pool_against_fp64(B, Q, C, H, W):
    plan = Fn.mask_pool_plan(B, Q, C, H, W)
    assert plan.slabs == -(-H * W // plan.slab)
    if (H, W) == THREE_SLABS:
        assert plan.slabs >= 3 and (H * W) % plan.slab not in (0,)
    x, logits = _pool_case(B, Q, C, H, W)
    total, count = _check_pool(x, logits, f"mask_pool {(B, Q, C, H, W)}")
    pooled, denorm = Fn.mask_pool_mean(x.to(DEV), logits.to(DEV))
    assert torch.equal(pooled, total / (count.float() + 1e-8).unsqueeze(-1)) and denorm.shape == (B, Q, 1, 1)


def test_mask_pool_strided_frames_equal_contiguous_copies():
    """A (1, Q, T, H, W) logit tensor pooled frame by frame through its strides, and all frames in one call through the (T, Q) view."""
    Q, T, C, H, W = 21, 3, 36, 9, 14
    x, logits = _rand(T, C, H, W, seed=3).to(DEV), _rand(1, Q, T, H, W, seed=4).to(DEV)
    want = [Fn.mask_pool(x[t:t + 1], logits[:, :, t].contiguous()) for t in range(T)]
    for t in range(T):
        view = logits[:, :, t]
        assert not view.is_contiguous()
        total, count = Fn.mask_pool(x[t:t + 1], view)
        assert torch.equal(total, want[t][0]) and torch.equal(count, want[t][1])
    total, count = Fn.mask_pool(x, logits[0].transpose(0, 1))                 # (T, Q, H, W): batch stride H W, query stride T H W
    assert torch.equal(total, torch.cat([w[0] for w in want])) and torch.equal(count, torch.cat([w[1] for w in want]))
    with pytest.raises(RuntimeError, match="planes of mask_logits must be contiguous"):
        Fn.mask_pool(x[:1], logits[:, :, 0].transpose(-1, -2).contiguous().transpose(-1, -2))


def test_mask_pool_empty_full_and_threshold_rows():
    B, Q, C, H, W = 2, 6, 12, 7, 9
    x, logits = _pool_case(B, Q, C, H, W, seed=7)
    logits[:, 0] = -1.0                                                       # no pixel
    logits[:, 1] = 2.0                                                        # every pixel
    logits[:, 2] = torch.tensor([0.0, -0.0, 1e-45, float("nan"), -1e-45, 1.0, float("inf"), -float("inf"), 3.0]).repeat(H, 1)
    total, count = Fn.mask_pool(x.to(DEV), logits.to(DEV))
    assert torch.equal(total[:, 0], torch.zeros(B, C, device=DEV)) and count[:, 0].tolist() == [0, 0]
    pooled = Fn.mask_pool_mean(x.to(DEV), logits.to(DEV))[0]
    assert torch.equal(pooled[:, 0], torch.zeros(B, C, device=DEV))
    assert count[:, 1].tolist() == [H * W] * 2
    torch.testing.assert_close(total[:, 1].cpu().double(), x.double().sum((-1, -2)), rtol=1e-5, atol=1e-5)
    assert count[:, 2].tolist() == [4 * H] * 2                                # the denormal, 1.0, inf and 3.0 columns
    want = x.double()[..., [2, 5, 6, 8]].sum((-1, -2))
    torch.testing.assert_close(total[:, 2].cpu().double(), want, rtol=1e-5, atol=1e-5)
    s64, c64 = cpu_ops.mask_pool(x.double(), logits.double())
    assert torch.equal(count.cpu(), c64)


def test_mask_pool_bits():
    B, Q, C, H, W = 3, 19, 24, 70, 61                                         # 2 slabs, unaligned
    x, logits = (t.to(DEV) for t in _pool_case(B, Q, C, H, W, seed=11))
    first = Fn.mask_pool(x, logits)
    again = Fn.mask_pool(x, logits)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])             # two calls, equal bits
    alone = Fn.mask_pool(x[1:2].contiguous(), logits[1:2].contiguous())
    assert torch.equal(alone[0], first[0][1:2]) and torch.equal(alone[1], first[1][1:2])   # a frame alone / in a batch of 3
    poisoned = x.clone()
    poisoned[1, 5, 3, 3] = float("nan")
    got = Fn.mask_pool(poisoned, logits)
    assert torch.equal(got[0][[0, 2]], first[0][[0, 2]]) and torch.equal(got[1], first[1])  # the other frames: bit-equal


def test_mask_pool_overwrites_its_outputs(monkeypatch):
    """Sentinel-filled outputs are fully overwritten: torch.empty is replaced by a NaN / -7 fill for the call."""
    real = torch.empty

    def filled(*a, **k):
        t = real(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(-7)
    for shape in ((2, 5, 20, 3, 5), (2, 18, 260, 70, 61)):
        x, logits = (t.to(DEV) for t in _pool_case(*shape, seed=13))
        monkeypatch.setattr(torch, "empty", filled)
        total, count = Fn.mask_pool(x, logits)
        monkeypatch.setattr(torch, "empty", real)
        assert torch.isfinite(total).all() and (count >= 0).all()
        s64, c64 = cpu_ops.mask_pool(x.cpu().double(), logits.cpu().double())
        assert torch.equal(count.cpu(), c64)
        torch.testing.assert_close(total.cpu().double(), s64, rtol=1e-4, atol=1e-4)


def test_ops_refuse_a_backward():
    x, logits = (t.to(DEV) for t in _pool_case(1, 3, 4, 5, 7))
    with pytest.raises(RuntimeError, match="no backward for mask_pool"):
        Fn.mask_pool(x.requires_grad_(), logits)
    emb, text = _rand(3, 8).to(DEV).requires_grad_(), _rand(4, 8, seed=1).to(DEV)
    with pytest.raises(RuntimeError, match="no backward for text_class_logits"):
        Fn.text_class_logits(emb, text, torch.tensor(1.0, device=DEV), [3, 1])
    with pytest.raises(RuntimeError, match="no backward for ov_ensemble"):
        Fn.ov_ensemble(_rand(2, 4).to(DEV).requires_grad_(), _rand(2, 4).to(DEV), torch.ones(3), 0.4, 0.8)
    with torch.no_grad():
        assert Fn.mask_pool(x, logits)[0].shape == (1, 3, 4)


# ---------------------------------------------------------------------------------------------------------- text_class_logits
def _segments(n, total, seed):
    """n segment lengths >= 1 adding up to `total`, mixed."""
    g = torch.Generator().manual_seed(seed)
    cuts = torch.randperm(total - 1, generator=g)[:n - 1].add(1).sort().values.tolist()
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


def _check_text(x, text, scale, templates, what):
    s = torch.tensor(float(scale))
    got = Fn.text_class_logits(x.to(DEV), text.to(DEV), s.to(DEV), templates)
    c32 = cpu_ops.text_class_logits(x, text, s, templates)
    c64 = cpu_ops.text_class_logits(x.double(), text.double(), s.double(), templates)
    assert got.shape == c64.shape and torch.isfinite(got).all()
    check_4x({"logits": got}, {"logits": c32}, {"logits": c64}, what + " ")
    return got, c32, c64


@pytest.mark.parametrize("R,D,N,templates", [(1, 4, 2, [1, 1]), (7, 24, 11, [3, 1, 2, 4, 1]), (130, 768, 600, None)])
def test_text_class_logits_against_fp64(R, D, N, templates):
    templates = templates or _segments(41, N, seed=2)
    assert len(templates) in (2, 5, 41) and sum(templates) == N
    x, text = _rand(R, D, seed=20), torch.nn.functional.normalize(_rand(N, D, seed=21), dim=-1)
    _check_text(x, text, math.log(1 / 0.07), templates, f"text_class_logits {(R, D, N)}")


def test_text_class_logits_edges():
    R, D, templates = 9, 24, [3, 1, 2, 4, 1]
    x, text = _rand(R, D, seed=22), torch.nn.functional.normalize(_rand(11, D, seed=23), dim=-1)
    text[5] = torch.nn.functional.normalize(x[0], dim=-1)                     # segment 2 = rows 4, 5: its maximum is its LAST row
    x[3] = 0.0                                                                # a zero row: finite, and the CPU's value
    got, c32, _ = _check_text(x, text, math.log(1 / 0.07), templates, "edges")
    assert torch.isclose(got[0, 2].cpu(), torch.tensor(x[0].norm().item() / x[0].norm().item() / 0.07), rtol=1e-4)
    assert torch.equal(got[3].cpu(), c32[3]) and torch.equal(got[3].cpu(), torch.zeros(5))
    hot, _, _ = _check_text(x, text, 5.0, templates, "clamped")               # exp(5) = 148 > 100: the clamp is active
    unit, _, _ = _check_text(x, text, 0.0, templates, "unit")
    torch.testing.assert_close(hot, 100 * unit, rtol=1e-5, atol=1e-4)
    batched = Fn.text_class_logits(x.view(3, 3, D).to(DEV), text.to(DEV), torch.tensor(5.0, device=DEV), templates)
    assert batched.shape == (3, 3, 5) and torch.equal(batched.view(9, 5), hot)


# ---------------------------------------------------------------------------------------------------------------- ov_ensemble
def _clip_logits(R, K, seed):
    """Logits at CLIP's natural scale: cosines x 100."""
    g = torch.Generator().manual_seed(seed)
    return 100 * (2 * torch.rand(R, K + 1, generator=g) - 1)


@pytest.mark.parametrize("K", [1, 5, 124, 1203])
@pytest.mark.parametrize("R", [1, 257])
def test_ov_ensemble_against_fp64(K, R):
    a, b = _clip_logits(R, K, 30), _clip_logits(R, K, 31)
    g = torch.Generator().manual_seed(32)
    valid = torch.randint(0, 3, (R,), generator=g, dtype=torch.int32)
    valid[0] = 0
    for name, ov in (("mixed", (torch.rand(K, generator=g) < 0.5).float()), ("none", torch.zeros(K)), ("all", torch.ones(K))):
        for v in (None, valid):
            got = Fn.ov_ensemble(a.to(DEV), b.to(DEV), ov.to(DEV), 0.4, 0.8, None if v is None else v.to(DEV))
            assert torch.isfinite(got).all() and (got >= math.log(1e-8) - 1e-6).all()
            c32 = cpu_ops.ov_ensemble(a, b, ov, 0.4, 0.8, v)
            ref = C.reference_ensemble(a.double(), b.double(), ov, 0.4, 0.8, v)        # the reference's formula, in fp64
            check_4x({"out": got}, {"out": c32}, {"out": ref}, f"ov_ensemble K={K} R={R} {name} valid={v is not None} ")
    # alpha = beta = 0: the in-vocabulary distribution with void re-attached
    got = Fn.ov_ensemble(a.to(DEV), b.to(DEV), torch.ones(K, device=DEV), 0.0, 0.0)
    a64 = a.double()
    p_void = a64.softmax(-1)[..., -1:]
    want = torch.log(torch.cat([a64[..., :-1].softmax(-1) * (1 - p_void), p_void], -1) + 1e-8)
    check_4x({"out": got}, {"out": cpu_ops.ov_ensemble(a, b, torch.ones(K), 0.0, 0.0)}, {"out": want}, f"ov_ensemble K={K} R={R} a=0 ")


def test_ov_ensemble_shapes_and_refusals():
    a, b = _clip_logits(12, 5, 33).view(2, 6, 6).to(DEV), _clip_logits(12, 5, 34).view(2, 6, 6).to(DEV)
    valid = torch.tensor([[1, 0, 2, 0, 3, 1], [0, 0, 1, 1, 1, 0]], device=DEV)
    got = Fn.ov_ensemble(a, b, torch.tensor([1, 0, 1, 1, 0], device=DEV), 0.4, 0.8, valid)      # any dtype for the flags
    want = cpu_ops.ov_ensemble(a.cpu(), b.cpu(), torch.tensor([1, 0, 1, 1, 0]), 0.4, 0.8, valid.cpu())
    assert got.shape == (2, 6, 6)
    torch.testing.assert_close(got.cpu(), want, rtol=1e-4, atol=1e-4)
    with pytest.raises(RuntimeError, match="K=2049"):
        Fn.ov_ensemble(torch.zeros(1, 2050, device=DEV), torch.zeros(1, 2050, device=DEV), torch.ones(2049), 0.4, 0.8)


# ------------------------------------------------------------------------------------------------------------------- decoders
def test_decoders_against_the_reference():
    g = C.g22()
    dec = C.build_decoder(g, DEV)
    tr, tr_pooled = C.run_decoder(g, dec, train=True, device=DEV)
    for i, (logits, masks) in enumerate(C.predictions(tr)):
        print(f"prediction {i}: masks max |diff| {(masks.cpu() - g.t(f'{i}/pred_masks', g.preds)).abs().max().item():.3e}, class logits "
              f"{(logits.cpu() - g.t(f'{i}/pred_logits', g.preds)).abs().max().item():.3e}, pooled "
              f"{(tr_pooled[i][0].cpu() - g.t(f'{i}/pooled', g.pooled)).abs().max().item():.3e}")
    C.check_train_outputs(g, tr, tr_pooled, TOL)
    ev, ev_pooled = C.run_decoder(g, dec, train=False, device=DEV)
    C.check_eval_outputs(g, ev, TOL)
    # the eval output is the last prediction of the .train() / no_grad output, bit for bit
    assert torch.equal(ev["pred_logits"][0], tr["pred_logits"].flatten(0, 1))
    assert torch.equal(ev["pred_masks"][0].transpose(0, 1), tr["pred_masks"].transpose(1, 2).flatten(0, 1))
    assert torch.equal(ev["pred_embds"][0], tr["pred_embds"].permute(1, 0, 2, 3).flatten(1, 2))
    assert torch.equal(ev_pooled[0][0], tr_pooled[-1][0]) and torch.equal(ev_pooled[0][1], tr_pooled[-1][1])
    mv, _ = C.run_decoder(g, C.build_decoder(g, DEV, cls=C.MINVIS_OV), train=False, device=DEV)
    assert "mask_features" not in mv and torch.equal(mv["pred_logits"], ev["pred_logits"])
    dec.train()
    x, mf, text = g.inputs(DEV)
    with pytest.raises(NotImplementedError, match="no.*backward"):
        dec(x, mf, None, text_classifier=text, num_templates=g.templates)
