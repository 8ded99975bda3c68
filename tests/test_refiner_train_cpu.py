"""The refiner training stage on CPU tensors against g16 (the reference's TemporalRefiner in training mode, its criterion on the
(T h, w) reshape and its contrastive loss with the class-reference memory, two consecutive steps), and DVIS_Plus_offline in
.train() on the toy backbone.  Tolerances: TOL / TIGHT of test_tracker_train_gpu.py."""
import numpy as np
import pytest
import torch

from refiner_train_cases import (G16, STEPS, check_against_golden, check_offline_eval_after_training, check_offline_training,
                                 replay_shuffles, train_steps)

TOL = dict(rtol=1e-3, atol=1e-3)         # tests/test_golden_gpu.py, g4 tracker outputs: the contract ...
TIGHT = dict(rtol=2e-4, atol=5e-5)       # ... and its regression guard


@pytest.fixture(scope="module")
def g16():
    return G16()


@pytest.fixture(scope="module")
def steps(g16):
    return train_steps(g16, "cpu")[1]


def test_two_training_steps_vs_reference(g16, steps):
    check_against_golden(g16, steps, (TOL, TIGHT))
    out = steps[0]["out"]
    m = g16.meta
    assert out["pred_logits"].shape == (1, m["T"], m["Q"], m["classes"] + 1)
    assert out["pred_masks"].shape == (1, m["Q"], m["T"], m["H"], m["W"])
    assert out["pred_embds"].shape == (1, m["hidden"], m["T"], m["Q"])
    assert len(out["aux_outputs"]) == m["layers"] - 1 and set(out["aux_outputs"][0]) == {"pred_logits", "pred_masks"}
    assert out["pred_masks"].requires_grad and out["pred_logits"].requires_grad


def test_fixture_has_class_items_and_a_trimmed_memory(g16):
    m = g16.meta
    assert m["steps"][1]["memory_before"] == {} and m["steps"][2]["memory_before"]
    assert m["steps"][1]["n_shuffles"] >= 1 and m["steps"][2]["n_shuffles"] >= 1
    assert all(n <= m["max_len"] for s in STEPS for n in m["steps"][s]["memory_after"].values())
    labels = g16.z["in/tgt_labels"]
    assert len(labels) == 3 and len(set(labels.tolist())) == 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_contrastive_loss_of_step_2_on_recorded_inputs(g16, dtype):
    """The recorded embeddings, match and memory of step 1 in, the recorded losses and memory of step 2 out: class items present,
    memory trimmed.  On the recorded bits the memory must come out bit-equal."""
    from dvis_plus_amd.criterion import Outputs_Memory_PerClasses, refiner_contrastive_loss
    memory = Outputs_Memory_PerClasses(max_len=g16.meta["max_len"])
    memory.class_references = {c: list(rows.unbind(0)) for c, rows in g16.memory(1).items()}
    left = replay_shuffles(memory, g16.shuffles(2))
    embds = g16.t("step2/pred_embds")[0].permute(1, 2, 0).to(dtype).requires_grad_()
    match = tuple(torch.from_numpy(r.copy()) for r in g16.z["step2/match_idx"])
    got = refiner_contrastive_loss(embds, match, g16.t("in/tgt_labels"), memory)
    assert not left
    tol = dict(rtol=1e-5, atol=1e-7) if dtype == torch.float32 else dict(rtol=2e-6, atol=1e-8)      # fp32 recorded values
    for k in ("loss_reid", "loss_aux_reid"):
        torch.testing.assert_close(got[k].detach().float(), g16.t(f"step2/loss/{k}"), **tol)
    want = g16.memory(2)
    assert set(want) == set(memory.class_references)
    for c, rows in want.items():
        assert torch.equal(torch.stack(memory.class_references[c]).float(), rows)
        assert not memory.class_references[c][0].requires_grad
    got["loss_reid"].backward()
    assert embds.grad is not None and embds.grad.abs().max() > 0


def test_contrastive_loss_without_a_match_is_a_zero_with_a_graph():
    from dvis_plus_amd.criterion import Outputs_Memory_PerClasses, refiner_contrastive_loss
    embds = torch.randn(3, 4, 8, requires_grad=True)
    empty = torch.zeros(0, dtype=torch.int64)
    memory = Outputs_Memory_PerClasses(max_len=20)
    out = refiner_contrastive_loss(embds, (empty, empty), empty, memory)
    assert set(out) == {"loss_reid", "loss_aux_reid"}
    assert all(float(v.detach()) == 0 and v.requires_grad for v in out.values())
    (out["loss_reid"] + out["loss_aux_reid"]).backward()
    assert embds.grad is not None and embds.grad.abs().max() == 0
    assert memory.class_references == {} and memory.get_items(3) == []


def test_memory_shuffles_and_trims_through_its_hook():
    from dvis_plus_amd.criterion import Outputs_Memory_PerClasses
    memory = Outputs_Memory_PerClasses(max_len=3)
    asked = []
    memory._draw = lambda kind, n: asked.append((kind, n)) or list(range(n))[::-1]
    refs = torch.arange(2 * 3 * 1, dtype=torch.float32).view(2, 3, 1)            # (T = 2, Q = 3, C = 1): value = 3 t + q
    memory.push_refiner(refs, {"labels": torch.tensor([7, 7])}, (torch.tensor([0, 2]), torch.tensor([0, 1])))
    assert asked == [("shuffle", 4)]                                             # rows 0, 3, 2, 5 -> reversed -> last three
    assert memory.get_items(7).flatten().tolist() == [2.0, 3.0, 0.0]
    assert len(Outputs_Memory_PerClasses(max_len=3)._draw("shuffle", 5)) == 5


def test_eval_path_is_untouched_by_the_training_branch(g16):
    from refiner_train_cases import build_refiner
    ref = build_refiner(g16).eval()
    ie, fe, mf = g16.inputs("cpu")
    with torch.no_grad():
        ev = ref(ie, fe, mf)
    assert ev["aux_outputs"] == [] and not ev["pred_masks"].requires_grad
    tr = ref.train()(ie, fe, mf)
    torch.testing.assert_close(tr["pred_masks"].detach(), ev["pred_masks"], **TIGHT)
    torch.testing.assert_close(tr["pred_logits"].detach(), ev["pred_logits"], **TIGHT)


def test_float64_module_stays_in_float64(g16):
    ref, steps = train_steps(g16, "cpu", torch.float64)
    assert steps[0]["out"]["pred_masks"].dtype == torch.float64
    assert all(v.dtype == torch.float64 for v in steps[1]["grads"].values())
    assert np.array_equal(torch.stack(steps[1]["match"][0]).numpy(), g16.z["step2/match_idx"])


def test_offline_model_training_forward():
    """DVIS_Plus_offline in .train() on the toy backbone with duck-typed instances: loss keys = the weight_dict's (with the
    contrastive key), finite, gradients for every refiner parameter and none for backbone, head or tracker, iter advances, the
    guide is matched on in the first half of the schedule and the refiner's own outputs after it, no criterion raises."""
    check_offline_training("cpu")


def test_offline_model_eval_after_a_training_call():
    """Eval on the same video after a training call = a model that never trained, bit for bit; weights unchanged."""
    check_offline_eval_after_training("cpu")
