"""csrc/mask_gemm_backward.hip: the mask-logit contraction's backward (grad_embed = g feat^T, row_sum = sum_p g), its
determinism, and the autograd wiring of functions.mask_logits / functions.projected_mask_logits.

Integer operands make every product and partial sum exact in fp32, so the result must be bit-equal to the fp64 einsum whatever
the summation order: that catches indexing, slab-edge and reduction errors without a tolerance.  For normal operands the bound
is measured, not chosen: the error of torch's own fp32 CPU einsum against fp64 on the same inputs, times 4 (a different
summation order over up to 58 880 terms)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, R, C, H, W): the production tile shape; R below one MFMA tile with HW odd (scalar loads); R = layers x queries over several
# row blocks; C no multiple of 32; the production map (15 pixel slabs and the second pass)
SHAPES = [(2, 100, 256, 8, 12), (1, 7, 256, 5, 7), (1, 600, 256, 16, 20), (2, 20, 48, 8, 12), (1, 100, 256, 184, 320)]


@pytest.fixture(scope="module")
def Fn():
    from dvis_plus_amd import functions
    return functions


def _integers(B, R, C, H, W, seed):
    """|x| <= 3, about one pixel in eight non-zero per operand: |sum| <= 9 * 58 880 < 2^24."""
    gen = torch.Generator().manual_seed(seed)

    def draw(*shape):
        v = torch.randint(-3, 4, shape, generator=gen).float()
        return v * (torch.rand(shape, generator=gen) < 0.125)
    return draw(B, R, H, W), draw(B, C, H, W)


def _ref64(g, feat):
    g64, f64 = g.double().flatten(2), feat.double().flatten(2)
    return torch.einsum("brp,bcp->brc", g64, f64), g64.sum(-1)


@pytest.mark.parametrize("B,R,C,H,W", SHAPES)
def test_backward_is_exact_on_integers(Fn, B, R, C, H, W):
    g, feat = _integers(B, R, C, H, W, 7)
    ge, rs = Fn.mask_logits_backward(g.cuda(), feat.cuda())
    ref_e, ref_s = _ref64(g, feat)
    assert ge.shape == (B, R, C) and rs.shape == (B, R)
    assert torch.equal(ge.cpu(), ref_e.float())
    assert torch.equal(rs.cpu(), ref_s.float())


def test_backward_on_views_with_an_offset_base(Fn):
    """Contiguous views whose first element is 4 bytes past a 16-byte boundary: the scalar-load form."""
    B, R, C, H, W = 2, 100, 256, 8, 12
    g, feat = _integers(B, R, C, H, W, 8)
    gbuf = torch.zeros(g.numel() + 1, device="cuda")
    fbuf = torch.zeros(feat.numel() + 1, device="cuda")
    gv, fv = gbuf[1:].view(g.shape), fbuf[1:].view(feat.shape)
    gv.copy_(g), fv.copy_(feat)
    assert gv.data_ptr() % 16 == 4 and fv.data_ptr() % 16 == 4
    ge, rs = Fn.mask_logits_backward(gv, fv)
    ref_e, ref_s = _ref64(g, feat)
    assert torch.equal(ge.cpu(), ref_e.float())
    assert torch.equal(rs.cpu(), ref_s.float())
    ge2, rs2 = Fn.mask_logits_backward(g.cuda(), fv)        # one aligned operand does not make the call vector-loadable
    assert torch.equal(ge2, ge) and torch.equal(rs2, rs)


def _bound(ref64, cpu32):
    """4 x the error of torch's fp32 CPU result against fp64 on the same inputs."""
    return 4 * (cpu32.double() - ref64).abs().max().item()


@pytest.mark.parametrize("B,R,C,H,W", SHAPES)
def test_backward_on_normal_operands_and_determinism(Fn, B, R, C, H, W):
    gen = torch.Generator().manual_seed(11)
    g, feat = torch.randn(B, R, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen)
    ref_e, ref_s = _ref64(g, feat)
    cpu_e = torch.einsum("brp,bcp->brc", g.flatten(2), feat.flatten(2))
    cpu_s = g.flatten(2).sum(-1)
    gd, fd = g.cuda(), feat.cuda()
    ge, rs = Fn.mask_logits_backward(gd, fd)
    err_e, err_s = (ge.cpu().double() - ref_e).abs().max().item(), (rs.cpu().double() - ref_s).abs().max().item()
    print(f"shape {(B, R, C, H, W)}: grad_embed err {err_e:.3e} (bound {_bound(ref_e, cpu_e):.3e}), "
          f"row_sum err {err_s:.3e} (bound {_bound(ref_s, cpu_s):.3e})")
    assert err_e <= _bound(ref_e, cpu_e)
    assert err_s <= _bound(ref_s, cpu_s)
    # the same inputs give the same bits, and a frame's result does not depend on the batch it is part of
    ge2, rs2 = Fn.mask_logits_backward(gd, fd)
    assert torch.equal(ge, ge2) and torch.equal(rs, rs2)
    other_g, other_f = torch.randn_like(gd[:1]), torch.randn_like(fd[:1])
    ge3, rs3 = Fn.mask_logits_backward(torch.cat([other_g, gd[-1:]]), torch.cat([other_f, fd[-1:]]))
    ge1, rs1 = Fn.mask_logits_backward(gd[-1:].contiguous(), fd[-1:].contiguous())
    assert torch.equal(ge3[1], ge1[0]) and torch.equal(rs3[1], rs1[0])
    assert torch.equal(ge1[0], ge[-1]) and torch.equal(rs1[0], rs[-1])


def test_zero_rows_give_zero_rows(Fn):
    B, R, C, H, W = 1, 100, 256, 72, 64          # 4608 pixels: two slabs
    gen = torch.Generator().manual_seed(12)
    g, feat = torch.randn(B, R, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen)
    dead = torch.ones(R, dtype=torch.bool)
    dead[torch.arange(0, R, 10)] = False         # the criterion writes gradient into about a tenth of the rows
    g[:, dead] = 0
    ge, rs = Fn.mask_logits_backward(g.cuda(), feat.cuda())
    assert ge[:, dead.cuda()].abs().max().item() == 0 and rs[:, dead.cuda()].abs().max().item() == 0
    assert ge[:, ~dead.cuda()].abs().min().item() > 0


@pytest.mark.parametrize("embed_grad,feat_grad", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("B,Q,C,H,W", [(2, 100, 256, 8, 12), (1, 7, 48, 5, 7)])
def test_mask_logits_autograd(Fn, B, Q, C, H, W, embed_grad, feat_grad):
    gen = torch.Generator().manual_seed(13)
    e, f, go = torch.randn(B, Q, C, generator=gen), torch.randn(B, C, H, W, generator=gen), torch.randn(B, Q, H, W, generator=gen)

    def run(e, f, einsum):
        e, f = e.clone().requires_grad_(embed_grad), f.clone().requires_grad_(feat_grad)
        out = torch.einsum("bqc,bchw->bqhw", e, f) if einsum else Fn.mask_logits(e, f)
        out.backward(go.to(out))
        return out.detach(), e.grad, f.grad
    out, ge, gf = run(e.cuda(), f.cuda(), False)
    out64, ge64, gf64 = run(e.double(), f.double(), True)
    out32, ge32, gf32 = run(e, f, True)
    assert (ge is not None) == embed_grad and (gf is not None) == feat_grad
    for got, ref, cpu in ((out, out64, out32), (ge, ge64, ge32), (gf, gf64, gf32)):
        if got is not None:
            assert (got.cpu().double() - ref).abs().max().item() <= _bound(ref, cpu)
    with torch.no_grad():
        plain = Fn.mask_logits(e.cuda(), f.cuda())
    assert torch.equal(Fn.mask_logits(e.cuda(), f.cuda()), plain)      # nothing requires grad: today's call
    assert torch.equal(out, plain)                                      # and the autograd form runs the same forward kernel


def test_mask_logits_feature_gradient_refuses_more_than_256_rows(Fn):
    e = torch.randn(1, 300, 64, device="cuda")
    f = torch.randn(1, 64, 4, 8, device="cuda", requires_grad=True)
    out = Fn.mask_logits(e, f)
    with pytest.raises(RuntimeError, match="256"):
        out.sum().backward()


def test_projected_mask_logits_autograd(Fn):
    """mask_embed . (W feat + b) and its gradients for mask_embed, W, b against the fp64 project-then-contract form."""
    B, R, C, H, W = 2, 24, 64, 6, 10
    gen = torch.Generator().manual_seed(14)
    e, f = torch.randn(B, R, C, generator=gen), torch.randn(B, C, H, W, generator=gen)
    w, b = torch.randn(C, C, 1, 1, generator=gen) / 8, torch.randn(C, generator=gen)
    go = torch.randn(B, R, H, W, generator=gen)

    def run(e, f, w, b, fused):
        e, w, b = e.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        if fused:
            out = Fn.projected_mask_logits(e, f, w, b)
        else:
            out = torch.einsum("bqc,bchw->bqhw", e, torch.nn.functional.conv2d(f, w, b))
        out.backward(go.to(out))
        return out.detach(), e.grad, w.grad, b.grad
    got = run(e.cuda(), f.cuda(), w.cuda(), b.cuda(), True)
    ref = run(e.double(), f.double(), w.double(), b.double(), False)
    cpu = run(e, f, w, b, False)
    for x, r, c in zip(got, ref, cpu):
        assert x.shape == r.shape
        assert (x.cpu().double() - r).abs().max().item() <= _bound(r, c)
    with torch.no_grad():
        assert torch.equal(Fn.projected_mask_logits(e.cuda(), f.cuda(), w.cuda(), b.cuda()), got[0])
    with pytest.raises(RuntimeError, match="frozen"):
        Fn.projected_mask_logits(e.cuda().requires_grad_(), f.cuda().requires_grad_(), w.cuda(), b.cuda()).sum().backward()


def test_backward_refuses_what_it_cannot_address(Fn):
    with pytest.raises(RuntimeError, match="C <= 256"):
        Fn.mask_logits_backward(torch.zeros(1, 4, 2, 2, device="cuda"), torch.zeros(1, 257, 2, 2, device="cuda"))
    with pytest.raises(RuntimeError, match="float32"):
        Fn.mask_logits_backward(torch.zeros(1, 4, 2, 2, device="cuda", dtype=torch.float64), torch.zeros(1, 8, 2, 2, device="cuda"))
    with pytest.raises(RuntimeError, match="disagree"):
        Fn.mask_logits_backward(torch.zeros(1, 4, 2, 3, device="cuda"), torch.zeros(1, 8, 2, 2, device="cuda"))
