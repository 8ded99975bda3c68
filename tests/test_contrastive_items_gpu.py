"""The contrastive-items kernels (csrc/contrastive_items.hip, Fn.contrastive_items / Fn.contrastive_items_backward) against the fp64
CPU autograd of the reference's per-item composition under the project's rule (ctvis_cases.check_4x: 4 x the fp32 CPU run's own
distance where a tensor has >= MIN_SAMPLES elements, rtol 2e-3 / atol 5e-4 below), and the planted cases."""
import ctypes

import pytest
import torch

import ctvis_cases as K
from dvis_plus_amd import functions as Fn
from dvis_plus_amd import native

pytestmark = pytest.mark.gpu
DEV = "cuda"


def run_kernels(src, lists, g_reid, g_aux):
    src = src.to(DEV)
    reid, aux, saved = Fn.contrastive_items(src, *lists, return_saved=True)
    grad = Fn.contrastive_items_backward(src, *lists, saved, g_reid.to(DEV), g_aux.to(DEV))
    return {"reid": reid, "aux": aux, "grad_src": grad}


def of_case(case, **kw):
    args = dict(src=case["src"], lists=case["lists"], g_reid=case["g_reid"], g_aux=case["g_aux"])
    args.update(kw)
    return run_kernels(**args)


def references(src, lists, g_reid, g_aux):
    return (K.composition_reference(src, lists, g_reid, g_aux, torch.float32),
            K.composition_reference(src, lists, g_reid, g_aux, torch.float64))


@pytest.mark.parametrize("name", sorted(K.OP_CASES))
def test_forward_and_backward_against_fp64(name):
    case = K.op_case(name)
    K.check_4x(of_case(case), case["cpu32"], case["cpu64"], f"{name} ")


def test_the_tile_case_exceeds_one_workgroup_pass():
    case = K.op_case("over_tile")
    slots = (case["lists"][1][1:] - case["lists"][1][:-1]) + (case["lists"][3][1:] - case["lists"][3][:-1])
    assert int(slots.min()) > K.tile() >= 64


def test_unreferenced_rows_get_exact_zeros_whatever_they_hold():
    case = K.op_case("planted")
    clean = of_case(case)
    src = case["src"].clone()
    src[10], src[11] = float("inf"), float("nan")
    got = of_case(case, src=src)
    assert torch.equal(got["grad_src"][10:], torch.zeros(2, case["C"], device=DEV))
    assert torch.equal(got["grad_src"][:10], clean["grad_src"][:10]) and torch.equal(got["reid"], clean["reid"])
    assert torch.equal(clean["grad_src"][10:], torch.zeros(2, case["C"], device=DEV))


def test_zero_negative_row():
    case = K.op_case("planted")
    src = case["src"].clone()
    src[6] = 0                                                # a negative of item 2: cosine 0, a finite gradient
    got = of_case(case, src=src)
    cpu32, cpu64 = references(src, case["lists"], case["g_reid"], case["g_aux"])
    assert torch.isfinite(got["grad_src"]).all() and torch.isfinite(cpu64["grad_src"]).all()
    K.check_4x(got, cpu32, cpu64, "zero negative row ")
    torch.testing.assert_close(got["grad_src"][6].cpu().double(), cpu64["grad_src"][6], **K.SMALL)


def test_large_dots_do_not_overflow():
    case = K.big_dots_case()
    got = of_case(case)
    assert all(torch.isfinite(v).all() for v in got.values())
    K.check_4x(got, case["cpu32"], case["cpu64"], "big dots ")
    torch.testing.assert_close(got["reid"][:2].cpu(), torch.tensor([160.0, 2000.0]), rtol=1e-5, atol=0)       # linear in the margin
    assert float(got["reid"][3]) == 0.0


@pytest.mark.parametrize("which", ["reid only", "aux only"])
def test_one_upstream_gradient_zero(which):
    case = K.op_case("n37")
    zero = torch.zeros(case["n"])
    g_reid, g_aux = (case["g_reid"], zero) if which == "reid only" else (zero, case["g_aux"])
    got = of_case(case, g_reid=g_reid, g_aux=g_aux)
    cpu32, cpu64 = references(case["src"], case["lists"], g_reid, g_aux)
    K.check_4x(got, cpu32, cpu64, which + " ")
    assert float(got["grad_src"].abs().max()) > 0


def test_zero_upstream_gives_exact_zeros():
    case = K.op_case("n37")
    zero = torch.zeros(case["n"])
    got = of_case(case, g_reid=zero, g_aux=zero)
    assert torch.equal(got["grad_src"], torch.zeros_like(got["grad_src"]))


def test_a_nan_row_reaches_exactly_what_references_it():
    g = torch.Generator().manual_seed(77)
    R, C, bad = 30, 64, 4
    items = K.random_items(g, 12, R, (1, 2), (1, 5))
    items[0] = (bad, items[0][1], items[0][2])                 # as an anchor, a positive and a negative
    items[1] = (items[1][0], [bad], items[1][2])
    items[2] = (items[2][0], items[2][1], items[2][2] + [bad])
    lists = K.make_lists(items)
    src = torch.randn(R, C, generator=g) * 0.5
    g_reid, g_aux = torch.randn(12, generator=g), torch.randn(12, generator=g)
    clean = run_kernels(src, lists, g_reid, g_aux)
    src_nan = src.clone()
    src_nan[bad, 5] = float("nan")
    got = run_kernels(src_nan, lists, g_reid, g_aux)
    hit = [i for i, (a, p, n) in enumerate(items) if bad in [a] + p + n]
    rows = sorted({r for i in hit for r in [items[i][0]] + items[i][1] + items[i][2]})
    assert 3 <= len(hit) < 12 and len(rows) < R
    for k in ("reid", "aux"):
        assert (~torch.isfinite(got[k])).nonzero().flatten().tolist() == hit, k
    assert (~torch.isfinite(got["grad_src"])).any(1).nonzero().flatten().tolist() == rows
    ref = K.composition_reference(src_nan, lists, g_reid, g_aux, torch.float64)
    assert (~torch.isfinite(ref["reid"])).nonzero().flatten().tolist() == hit                # the fp64 composition agrees
    assert (~torch.isfinite(ref["grad_src"])).any(1).nonzero().flatten().tolist() == rows
    keep_items = [i for i in range(12) if i not in hit]
    assert torch.equal(got["reid"][keep_items], clean["reid"][keep_items]) and torch.equal(got["aux"][keep_items], clean["aux"][keep_items])
    untouched = [r for r in range(R) if not any(r in [items[i][0]] + items[i][1] + items[i][2] for i in hit)]
    assert torch.equal(got["grad_src"][untouched], clean["grad_src"][untouched])


def test_two_calls_give_the_same_bits():
    for name in ("n37", "N200", "over_tile", "C260"):
        case = K.op_case(name)
        a, b = of_case(case), of_case(case)
        assert all(torch.equal(a[k], b[k]) for k in a), name


def test_autograd_equals_the_explicit_backward():
    case = K.op_case("n37")
    explicit = of_case(case)
    src = case["src"].to(DEV).requires_grad_()
    with torch.no_grad():
        plain = Fn.contrastive_items(src, *case["lists"])
    reid, aux = Fn.contrastive_items(src, *case["lists"])
    assert reid.requires_grad and not plain[0].requires_grad
    assert torch.equal(reid, explicit["reid"]) and torch.equal(aux, explicit["aux"]) and torch.equal(plain[0], reid)
    ((reid * case["g_reid"].to(DEV)).sum() + (aux * case["g_aux"].to(DEV)).sum()).backward()
    assert torch.equal(src.grad, explicit["grad_src"])
    src2 = case["src"].to(DEV).requires_grad_()
    r2, a2 = Fn.contrastive_items(src2, *case["lists"])
    (g2,) = torch.autograd.grad([r2, a2], src2, [case["g_reid"].to(DEV), case["g_aux"].to(DEV)])
    assert torch.equal(g2, explicit["grad_src"])
    # through a cat and an index: the rows' gradients flow back to both parts
    x, y = case["src"][:20].to(DEV).requires_grad_(), case["src"][20:].to(DEV).requires_grad_()
    reid, aux = Fn.contrastive_items(torch.cat([x, y]), *case["lists"])
    ((reid * case["g_reid"].to(DEV)).sum() + (aux * case["g_aux"].to(DEV)).sum()).backward()
    assert torch.equal(torch.cat([x.grad, y.grad]), explicit["grad_src"])


def test_torch_formulation_switch(monkeypatch):
    case = K.op_case("n37")
    calls = []
    inner = native.lib().dvis_contrastive_items
    monkeypatch.setenv("DVIS_CONTRASTIVE_ITEMS", "0")
    monkeypatch.setattr(Fn, "_contrastive_items_kernel", lambda *a: calls.append(1))
    src = case["src"].to(DEV).requires_grad_()
    reid, aux = Fn.contrastive_items(src, *case["lists"])
    ((reid * case["g_reid"].to(DEV)).sum() + (aux * case["g_aux"].to(DEV)).sum()).backward()
    assert not calls and inner is not None
    K.check_4x({"reid": reid.detach(), "aux": aux.detach(), "grad_src": src.grad}, case["cpu32"], case["cpu64"], "torch formulation on the GPU ")


def test_no_items():
    e, z = torch.zeros(0, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    src = torch.randn(5, 8, device=DEV, requires_grad=True)
    reid, aux = Fn.contrastive_items(src, e, z, e, z, e)
    assert reid.shape == aux.shape == (0,) and reid.is_cuda and reid.dtype == torch.float32
    (reid.sum() + aux.sum()).backward()
    assert torch.equal(src.grad, torch.zeros_like(src))
    r, a, saved = Fn.contrastive_items(src.detach(), e, z, e, z, e, return_saved=True)
    g = Fn.contrastive_items_backward(src.detach(), e, z, e, z, e, saved, torch.zeros(0), torch.zeros(0))
    assert torch.equal(g, torch.zeros_like(src))


def test_wrapper_refusals_on_the_gpu():
    lists = K.make_lists([(0, [1], [2, 3])])
    with pytest.raises(RuntimeError, match="C % 4"):
        Fn.contrastive_items(torch.randn(6, 6, device=DEV), *lists)
    with pytest.raises(RuntimeError, match="contiguous"):
        Fn.contrastive_items(torch.randn(8, 6, device=DEV).t(), *lists)
    with pytest.raises(RuntimeError, match="float32"):
        Fn.contrastive_items(torch.randn(6, 8, device=DEV, dtype=torch.float64), *lists)
    with pytest.raises(RuntimeError, match="outside"):
        Fn.contrastive_items(torch.randn(3, 8, device=DEV), *lists)
    src = torch.randn(6, 8, device=DEV)
    _, _, saved = Fn.contrastive_items(src, *lists, return_saved=True)
    with pytest.raises(RuntimeError, match="saved"):
        Fn.contrastive_items_backward(src, *K.make_lists([(0, [1], [2, 3, 4, 5])]), saved, torch.zeros(1), torch.zeros(1))


GUARD = 64            # floats: 256 bytes, keeps the 16-byte alignment


def guarded(n, value=777.0):
    buf = torch.full((n + 2 * GUARD,), value, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def test_entry_points_guard_bands_and_error_codes():
    case = K.op_case("n37")
    lib = native.lib()
    R, C, n = case["R"], case["C"], case["n"]
    lists = [t.to(DEV) for t in case["lists"]]
    S = case["lists"][2].numel() + case["lists"][4].numel()
    tr = [t.to(DEV) for t in Fn.contrastive_items_transpose(*case["lists"], R)]
    src = case["src"].to(DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = native.stream_ptr(torch.device(DEV))
    (b_reid, reid), (b_aux, aux), (b_dots, dots), (b_norms, norms), (b_stats, stats) = (guarded(k) for k in (n, n, S, S, 3 * n))

    def forward(src_=src, C_=C, reid_=reid, anchor_=lists[0]):
        return lib.dvis_contrastive_items(p(src_) if src_ is not None else None, R, C_, p(anchor_), p(lists[1]), p(lists[2]), p(lists[3]),
                                          p(lists[4]), n, S, p(reid_), p(aux), p(dots), p(norms), p(stats), stream)
    assert forward() == 0
    want = of_case(case)
    assert torch.equal(reid, want["reid"]) and torch.equal(aux, want["aux"])
    for buf, k in ((b_reid, n), (b_aux, n), (b_dots, S), (b_norms, S), (b_stats, 3 * n)):
        assert bool((buf[:GUARD] == 777.0).all()) and bool((buf[GUARD + k:] == 777.0).all())
    nbytes = lib.dvis_contrastive_items_backward_ws_bytes(n, S, C)
    assert nbytes == 4 * ((2 * S + n + 3) // 4 * 4 + n * C)
    assert lib.dvis_contrastive_items_backward_ws_bytes(n, S, 6) == -1 and lib.dvis_contrastive_items_backward_ws_bytes(-1, S, C) == -1
    b_ws, ws = guarded(nbytes // 4)
    b_grad, grad = guarded(R * C)
    g_reid, g_aux = case["g_reid"].to(DEV), case["g_aux"].to(DEV)

    def backward(grad_=grad, ws_=ws, C_=C):
        return lib.dvis_contrastive_items_backward(p(src), R, C_, *(p(t) for t in lists), n, S, *(p(t) for t in tr), p(dots), p(norms),
                                                   p(stats), p(g_reid), p(g_aux), p(grad_), p(ws_) if ws_ is not None else None, stream)
    assert backward() == 0
    assert torch.equal(grad.view(R, C), want["grad_src"])
    for buf, k in ((b_ws, nbytes // 4), (b_grad, R * C)):
        assert bool((buf[:GUARD] == 777.0).all()) and bool((buf[GUARD + k:] == 777.0).all())
    for what, rc in (("null src", forward(src_=None)), ("C % 4", forward(C_=6)), ("misaligned src", forward(src_=src.view(-1)[1:])),
                     ("misaligned reid", lib.dvis_contrastive_items(p(src), R, C, p(lists[0]), p(lists[1]), p(lists[2]), p(lists[3]),
                                                                    p(lists[4]), n, S, ctypes.c_void_p(reid.data_ptr() + 2), p(aux), p(dots),
                                                                    p(norms), p(stats), stream))):
        assert rc != 0 and b"contrastive_items" in lib.dvis_last_error(), what
    for what, rc in (("null ws", backward(ws_=None)), ("C % 4", backward(C_=6)), ("misaligned grad_src", backward(grad_=grad[1:])),
                     ("grad_src aliases src", backward(grad_=src))):
        assert rc != 0 and b"contrastive_items_backward" in lib.dvis_last_error(), what
    torch.cuda.synchronize()
