"""Shared helpers of test_refiner_train_cpu.py / test_refiner_train_gpu.py: the g16 fixture (the reference's temporal refiner in
training mode over two consecutive steps, gen_refiner_train_golden.py), replay of its recorded random draws, the two training
steps of the package's refiner + criterion + contrastive loss on it, and DVIS_Plus_offline in .train() on the toy backbone."""
import ast
import os

import numpy as np
import torch

from criterion_cases import Replay
from tracker_train_cases import BitMasks, Instances, matcher_calls, same_output

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEPS = (1, 2)


class G16:
    def __init__(self):
        self.z = np.load(os.path.join(GOLDEN, "g16_refiner_train.npz"))
        self.meta = ast.literal_eval(str(self.z["meta"]))      # repr() of a plain dict written by gen_refiner_train_golden.py
        self._grads = {}

    def t(self, name):
        return torch.from_numpy(self.z[name].copy())

    def state(self):
        z = np.load(os.path.join(GOLDEN, "g16_refiner_train_state.npz"))
        return {k: torch.from_numpy(z[k].copy()) for k in z.files}

    def grads(self, step):
        if step not in self._grads:
            z = np.load(os.path.join(GOLDEN, f"g16_refiner_train_grads_{step}.npz"))
            self._grads[step] = {k: torch.from_numpy(z[k].copy()) for k in z.files}
        return self._grads[step]

    def _series(self, step, prefix):
        return [self.z[n] for n in sorted(k for k in self.z.files if k.startswith(f"step{step}/{prefix}_"))]

    def crit_draws(self, step):
        return [torch.from_numpy(d.copy()) for d in self._series(step, "crit_draw")]

    def shuffles(self, step):
        return self._series(step, "shuffle")

    def memory(self, step):
        """{class: rows} after `step`."""
        pre = f"step{step}/memory/"
        return {int(k[len(pre):]): self.t(k) for k in self.z.files if k.startswith(pre)}

    def inputs(self, device, dtype=torch.float32):
        return tuple(self.t(f"in/{k}").to(device, dtype) for k in ("instance_embeds", "frame_embeds", "mask_features"))


def replay_shuffles(memory, shuffles):
    """Make `memory` hand back the recorded permutations in order, checking the length it asks for."""
    pending = list(shuffles)

    def _draw(kind, n):
        assert kind == "shuffle" and pending, (kind, len(pending))
        v = pending.pop(0)
        assert len(v) == n, (len(v), n)
        return [int(i) for i in v]
    memory._draw = _draw
    return pending


def build_refiner(g, device="cpu"):
    from dvis_plus_amd.refiner import TemporalRefiner
    m = g.meta
    ref = TemporalRefiner(hidden_channel=m["hidden"], feedforward_channel=m["ffn"], num_head=m["heads"],
                          decoder_layer_num=m["layers"], mask_dim=m["hidden"], class_num=m["classes"])
    ref.load_state_dict(g.state(), strict=True)
    return ref.to(device)


def build_criterion(g, device="cpu"):
    from dvis_plus_amd.criterion import VideoSetCriterion
    from dvis_plus_amd.matcher import VideoHungarianMatcher
    m = g.meta
    points = m["K"] * m["T"]                      # build_criterion(cfg, "DVIS_Plus_offline"): T times the points of a frame
    matcher = VideoHungarianMatcher(num_points=points, **m["weights"])
    return VideoSetCriterion(m["classes"], matcher=matcher, weight_dict=m["weight_dict"], eos_coef=0.1, losses=["labels", "masks"],
                             num_points=points, oversample_ratio=3.0, importance_sample_ratio=0.75).to(device)


def loss_reshape(out, g, device):
    from dvis_plus_amd.meta_architecture import DVIS_Plus_offline
    masks = g.t("in/tgt_masks").to(device, out["pred_masks"].dtype)
    targets = [{"labels": g.t("in/tgt_labels").to(device), "masks": masks}]
    _, o, targets = DVIS_Plus_offline.frame_decoder_loss_reshape(out, targets)
    return o, targets


def train_steps(g, device="cpu", dtype=torch.float32):
    """The two recorded steps: refiner forward in training mode, criterion with replayed draws, contrastive loss on one memory
    with replayed shuffles, backward of the weighted sum, the recorded SGD update.
    -> (refiner, [per step: dict(out, match, losses, grads, memory)])."""
    from dvis_plus_amd.criterion import Outputs_Memory_PerClasses, refiner_contrastive_loss
    ref = build_refiner(g, device).to(dtype).train()
    crit = build_criterion(g, device)
    memory = Outputs_Memory_PerClasses(max_len=g.meta["max_len"])
    ie, fe, mf = g.inputs(device, dtype)
    wd, steps = g.meta["weight_dict"], []
    for step in STEPS:
        ref.zero_grad()
        out = ref(ie, fe, mf)
        crit._rand = crit.matcher._rand = Replay(g.crit_draws(step))
        o2, targets = loss_reshape(out, g, device)
        losses, match = crit(o2, targets, ret_match_result=True)
        left = replay_shuffles(memory, g.shuffles(step))
        losses.update(refiner_contrastive_loss(o2["pred_embds"][0].permute(1, 2, 0), match[0], targets[0]["labels"], memory))
        assert not left, f"{len(left)} recorded shuffles were not asked for"
        sum(losses[k] * wd[k] for k in losses if k in wd).backward()
        steps.append(dict(out=out, match=match, losses={k: v.detach() for k, v in losses.items()},
                          grads={n: p.grad.detach().clone() for n, p in ref.named_parameters()},
                          memory={c: torch.stack(rows) for c, rows in memory.class_references.items()}))
        with torch.no_grad():
            for p in ref.parameters():
                p.sub_(g.meta["lr"] * p.grad)
    return ref, steps


def check_against_golden(g, steps, tols):
    """Matching indices equal; outputs of all layers, losses, every parameter's gradient and the memory within each of `tols`."""
    for step, s in zip(STEPS, steps):
        pre = f"step{step}/"
        assert np.array_equal(torch.stack(s["match"][0]).cpu().numpy(), g.z[pre + "match_idx"])
        assert set(s["losses"]) == set(g.meta["steps"][step]["loss_keys"])
        for tol in tols:
            for k in ("pred_logits", "pred_masks", "pred_embds"):
                torch.testing.assert_close(s["out"][k].detach().cpu().float(), g.t(pre + k), **tol)
            for i, a in enumerate(s["out"]["aux_outputs"]):
                for k in a:
                    torch.testing.assert_close(a[k].detach().cpu().float(), g.t(f"{pre}aux{i}/{k}"), **tol)
            for k, v in s["losses"].items():
                torch.testing.assert_close(v.cpu().float(), g.t(f"{pre}loss/{k}"), **tol, msg=lambda m, k=k: f"step {step} {k}: {m}")
            want = g.grads(step)
            assert set(want) == set(s["grads"])
            for n, v in s["grads"].items():
                torch.testing.assert_close(v.cpu().float(), want[n], **tol, msg=lambda m, n=n: f"step {step} {n}: {m}")
            mem = g.memory(step)
            assert set(mem) == set(s["memory"])
            for c, rows in s["memory"].items():
                torch.testing.assert_close(rows.cpu().float(), mem[c], **tol)


# ---- DVIS_Plus_offline in .train(): the g10 toy-backbone model with a criterion and duck-typed ground truth

def offline_model(device, use_cl=True, max_iter_num=2, T=3):
    """-> (model in .eval(), video dict with "instances", weight_dict).  3 instances; the last is absent (id -1) in every frame
    and must be dropped, the second is absent in frame 0; frame 1 hands its masks over as an object with `.tensor`."""
    import g10_model
    from dvis_plus_amd.criterion import VideoSetCriterion
    from dvis_plus_amd.matcher import VideoHungarianMatcher
    m, g, cfg, frames = g10_model.build("offline", "vps", device)
    wd = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    wd.update({f"{k}_{i}": v for i in range(cfg["refiner_layers"] - 1) for k, v in list(wd.items())[:3]})
    if use_cl:
        wd["loss_reid"] = 2.0
    matcher = VideoHungarianMatcher(num_points=64 * T, cost_class=2.0, cost_mask=5.0, cost_dice=5.0)
    m.criterion = VideoSetCriterion(cfg["K"], matcher=matcher, weight_dict=wd, eos_coef=0.1, losses=["labels", "masks"],
                                    num_points=64 * T, oversample_ratio=3.0, importance_sample_ratio=0.75).to(device)
    m.max_iter_num, m.use_cl = max_iter_num, use_cl
    video = g10_model.video(frames, cfg, 0, T, device=device)
    H, W = frames[0].shape[-2:]
    instances = []
    for f in range(T):
        masks = torch.zeros(3, H, W, dtype=torch.bool)
        masks[0, 2 + f:H // 2, 3:W // 2] = True
        masks[1, H // 2:, W // 3 + f:] = f > 0
        ids = torch.tensor([0, 1 if f > 0 else -1, -1])
        instances.append(Instances(ids, torch.tensor([1, 3, 2]), BitMasks(masks) if f == 1 else masks))
    video["instances"] = instances
    return m, video, wd


def check_offline_training(device):
    m, video, wd = offline_model(device)
    assert all(not p.requires_grad for p in m.tracker.parameters())         # frozen by the constructor
    calls = matcher_calls(m)
    m.train()
    losses = m([video])
    assert set(losses) == set(wd) and all(torch.isfinite(v).all() for v in losses.values())
    assert not m.backbone.training and not m.sem_seg_head.training and not m.tracker.training and m.refiner.training
    sum(losses.values()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.refiner.parameters())
    assert all(p.grad is None for mod in (m.backbone, m.sem_seg_head, m.tracker) for p in mod.parameters())
    assert m.iter == 1
    assert calls == [False], calls              # iter 0 < max_iter_num // 2: one match, on the tracker's (gradient-free) outputs
    assert m.classes_references_memory.class_references, "use_cl: the matched rows are pushed into the memory"
    del calls[:]
    again = m([video])                          # iter 1 >= max_iter_num // 2: every layer matched on the refiner's own outputs
    assert set(again) == set(wd) and m.iter == 2
    assert calls == [True] * m.refiner.num_layers, calls
    m.criterion = None
    try:
        m([video])
    except RuntimeError as e:
        assert "criterion" in str(e)
    else:
        raise AssertionError(".train() without a criterion must raise")


def check_offline_eval_after_training(device):
    m, video, _ = offline_model(device)
    fresh, _, _ = offline_model(device)
    weights = {k: v.clone() for k, v in m.state_dict().items()}
    first = m([video])                          # fills the caches and captures the graphs
    m.train()
    sum(m([video]).values()).backward()
    m.eval()
    after, want = m([video]), fresh([video])
    assert same_output(first, want) and same_output(after, want)
    now = m.state_dict()
    assert now.keys() == weights.keys() and all(torch.equal(now[k], weights[k]) for k in weights)
