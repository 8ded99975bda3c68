"""The contrastive-items op without a GPU: the host builder of the backward's transposed lists against a brute-force inversion,
the batched torch formulation (cpu_ops.contrastive_items) against the per-item composition in fp64, the separable softplus form
against the logsumexp over the padded pair matrix, and the wrapper's refusals."""
import pytest
import torch

import ctvis_cases as K
from dvis_plus_amd import cpu_ops
from dvis_plus_amd import functions as Fn


@pytest.mark.parametrize("seed", range(4))
def test_transposed_lists_equal_a_brute_force_inversion(seed):
    g = torch.Generator().manual_seed(seed)
    R = 7 + 5 * seed
    lists = K.make_lists(K.random_items(g, 3 + 9 * seed, R, (0, 3), (0, 6)))          # duplicates within a list, rows in several roles
    row_ptr, occ_slot, occ_item, arow_ptr, arow_item = Fn.contrastive_items_transpose(*lists, R)
    assert all(t.dtype == torch.int32 and not t.is_cuda for t in (row_ptr, occ_slot, occ_item, arow_ptr, arow_item))
    occ, roles = K.brute_force_transpose(lists, R)
    assert row_ptr.tolist() == [0] + torch.tensor([len(o) for o in occ]).cumsum(0).tolist()
    assert arow_ptr.tolist() == [0] + torch.tensor([len(o) for o in roles]).cumsum(0).tolist()
    for r in range(R):
        got = list(zip(occ_slot[row_ptr[r]:row_ptr[r + 1]].tolist(), occ_item[row_ptr[r]:row_ptr[r + 1]].tolist()))
        assert got == occ[r], r                                    # (item, slot) order = ascending global slot number
        assert arow_item[arow_ptr[r]:arow_ptr[r + 1]].tolist() == roles[r], r
    S = lists[2].numel() + lists[4].numel()
    assert sorted(occ_slot.tolist()) == list(range(S))


def test_transposed_lists_of_no_items():
    e = torch.zeros(0, dtype=torch.int32)
    z = torch.zeros(1, dtype=torch.int32)
    row_ptr, occ_slot, occ_item, arow_ptr, arow_item = Fn.contrastive_items_transpose(e, z, e, z, e, 5)
    assert row_ptr.tolist() == [0] * 6 and arow_ptr.tolist() == [0] * 6 and occ_slot.numel() == occ_item.numel() == arow_item.numel() == 0


@pytest.mark.parametrize("name", ["n37", "planted", "N0", "N200", "P5N3", "C260"])
def test_torch_formulation_equals_the_per_item_composition_in_fp64(name):
    case = K.op_case(name)
    src = case["src"].double().requires_grad_()
    reid, aux = cpu_ops.contrastive_items(src, *(t.long() for t in case["lists"]))
    (grad,) = torch.autograd.grad((reid * case["g_reid"].double()).sum() + (aux * case["g_aux"].double()).sum(), src)
    ref = case["cpu64"]
    torch.testing.assert_close(reid, ref["reid"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(aux, ref["aux"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(grad, ref["grad_src"], rtol=1e-11, atol=1e-12)
    # the dispatch: a CPU tensor takes this formulation, in its own dtype
    got = Fn.contrastive_items(case["src"].double(), *case["lists"])
    assert torch.equal(got[0], reid.detach()) and torch.equal(got[1], aux.detach())


def test_big_dots_do_not_overflow_in_the_torch_formulation():
    case = K.big_dots_case()
    reid, aux = cpu_ops.contrastive_items(case["src"], *(t.long() for t in case["lists"]))
    assert torch.isfinite(reid).all() and torch.isfinite(aux).all()
    torch.testing.assert_close(reid.double(), case["cpu64"]["reid"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(reid[:2].double(), torch.tensor([160.0, 2000.0], dtype=torch.float64), rtol=1e-5, atol=0)     # linear in the margin
    assert float(reid[2]) < 1e-30 and float(reid[3]) == 0.0


def test_separable_softplus_form_equals_logsumexp_over_the_padded_pair_matrix():
    g = torch.Generator().manual_seed(3)
    for P, N in ((1, 1), (1, 99), (5, 3), (3, 200)):
        dp, dn = torch.randn(P, generator=g, dtype=torch.float64) * 6, torch.randn(N, generator=g, dtype=torch.float64) * 6
        pairs = torch.nn.functional.pad((dn[None, :] - dp[:, None]).reshape(1, -1), (0, 1), "constant", 0)
        separable = torch.nn.functional.softplus(torch.logsumexp(dn, 0) + torch.logsumexp(-dp, 0), threshold=1e9)
        torch.testing.assert_close(separable, torch.logsumexp(pairs, dim=1)[0], rtol=1e-13, atol=1e-13)


def test_wrapper_refusals():
    src = torch.randn(6, 8)
    good = K.make_lists([(0, [1], [2, 3]), (4, [5], [0])])
    Fn.contrastive_items(src, *good)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    bad = {
        "row index outside": (good[0], good[1], i32([1, 6]), good[3], good[4]),
        "row index outside ": (i32([0, -1]), *good[1:]),
        "non-decreasing": (good[0], good[1], good[2], i32([0, 3, 2]), good[4]),
        "non-decreasing ": (good[0], i32([0, 1]), good[2], good[3], good[4]),                    # n + 1 entries
        "non-decreasing  ": (good[0], i32([1, 1, 2]), good[2], good[3], good[4]),                 # starts at 0
        "1-d int32 / int64": (good[0].float(), *good[1:]),
    }
    for what, lists in bad.items():
        with pytest.raises(RuntimeError, match=what.strip()):
            Fn.contrastive_items(src, *lists)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        Fn.contrastive_items(src, *good, return_saved=True)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        Fn.contrastive_items_backward(src, *good, None, torch.zeros(2), torch.zeros(2))
    e, z = torch.zeros(0, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    reid, aux = Fn.contrastive_items(src, e, z, e, z, e)
    assert reid.shape == aux.shape == (0,)
