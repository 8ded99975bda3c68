"""Writes tests/golden/g16_refiner_train.npz (+ g16_refiner_train_state.npz and g16_refiner_train_grads_{1,2}.npz: the split keeps
every file below the size limit) from the reference's own TemporalRefiner in TRAINING mode (dvis_Plus/refiner.py), its
VideoSetCriterion with VideoHungarianMatcher (mask2former_video/modeling/{criterion,matcher}.py) on the offline model's
(T h, w) reshape, and DVIS_Plus_offline.get_cl_loss_with_memory + loss_reid with Outputs_Memory_PerClasses
(dvis_Plus/meta_architecture.py, dvis_Plus/utils.py).

    python tests/golden/gen_refiner_train_golden.py

Build-machine only; nothing at test time imports this file.  The reference files are imported UNCHANGED through _ref_import.py
with the stubs of gen_criterion_golden.py and gen_tracker_train_golden.py.  The model's reshape between refiner and criterion
(DVIS_Plus_offline.frame_decoder_loss_reshape: 'b q t h w -> b q () (t h) w', pred_logits[:, 0]) is restated below with torch
ops.  Every random draw is recorded in order: torch.rand inside the criterion call (matcher and point sampling) and
random.shuffle inside the memory's push.

TWO consecutive steps on one model and one memory, a plain SGD update (meta["lr"]) between them: step 1 meets an empty memory
(instance items only) and its push already trims (max_len 6 < the 10 rows of the class that two instances share); step 2 has
class items and trims again.

Setup: hidden 64, 2 heads (d = 32), FFN 128, 2 layers, 5 classes, mask dim 64; T = 5 (the 5-tap convolution has an interior frame
and clamped edges), Q = 8, a 12 x 20 map, 3 ground-truth instances, two of them of one class; 64 points per frame.  Fixture
condition, as in g14 / g15: every assignment used is unchanged when its cost matrix is perturbed by Gaussian noise of sigma 5e-3.
"""
import os
import random
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_import as R    # noqa: E402
import gen_criterion_golden as G14    # noqa: E402
import gen_tracker_train_golden as G15    # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "g16_refiner_train{}.npz")
HID, HEADS, FFN, LAYERS, NCLS, T, Q, H, W, G, K = 64, 2, 128, 2, 5, 5, 8, 12, 20, 3, 64
WEIGHTS = dict(cost_class=2.0, cost_mask=5.0, cost_dice=5.0)
MAX_LEN, LR, STEPS = 6, 0.05, 2


class ShuffleRecorder:
    """random.shuffle replaced while active by a wrapper that draws the same permutation and records it as indices."""

    def __init__(self):
        self.draws = []

    def __enter__(self):
        self._orig = random.shuffle

        def shuffle(x):
            order = list(range(len(x)))
            self._orig(order)                  # the permutation random.shuffle(x) applies in this generator state
            x[:] = [x[i] for i in order]
            self.draws.append(np.array(order, dtype=np.int64))
        random.shuffle = shuffle
        return self

    def __exit__(self, *exc):
        random.shuffle = self._orig


def inputs():
    gen = torch.Generator().manual_seed(1600)
    base = torch.randn(Q, HID, generator=gen)
    instance = torch.stack([base + 0.05 * torch.randn(Q, HID, generator=gen) for _ in range(T)])       # (t, q, c): aligned
    frame = torch.stack([base[torch.randperm(Q, generator=gen)] + 0.05 * torch.randn(Q, HID, generator=gen) for _ in range(T)])
    to_bctq = lambda z: z.permute(2, 0, 1).unsqueeze(0).contiguous()
    mask_features = torch.randn(1, T, HID, H, W, generator=gen)
    tgt_masks = G14.boxes(gen, G, T, 2 * H, 2 * W).float()                  # (g, t, 24, 40)
    labels = torch.tensor([3, 1, 3])                                        # two instances of one class
    return to_bctq(instance), to_bctq(frame), mask_features, tgt_masks, labels


def loss_reshape(outputs, tgt_masks, labels):
    def one(d):
        b, q, t, h, w = d["pred_masks"].shape
        return {"pred_masks": d["pred_masks"].reshape(b, q, 1, t * h, w), "pred_logits": d["pred_logits"][:, 0]}
    out = one(outputs)
    out["pred_embds"] = outputs["pred_embds"]
    out["aux_outputs"] = [one(a) for a in outputs["aux_outputs"]]
    g, t, h, w = tgt_masks.shape
    return out, [{"labels": labels, "masks": tgt_masks.reshape(g, 1, t * h, w)}]


def main():
    """A randomly initialised refiner gives the matcher near-ties for most weight seeds: take the first seed from 1601 on at
    which the fixture condition holds in both steps."""
    G14.install()
    for seed in range(1601, 1901):
        try:
            return generate(seed)
        except AssertionError as e:
            if "fixture condition" not in str(e):
                raise
            print("seed", seed, ":", e)
    raise SystemExit("no seed met the fixture condition")


def generate(seed):
    ref_mod = R.ref("dvis_Plus.refiner")
    utils_mod = R.ref("dvis_Plus.utils")
    vm = R.ref("mask2former_video.modeling.matcher")
    vc = R.ref("mask2former_video.modeling.criterion")
    meta_mod = G15.ref_meta()
    spy = G14.CostSpy()
    vm.linear_sum_assignment = spy
    instance, frame, mask_features, tgt_masks, labels = inputs()
    wd = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    wd.update({f"{k}_{i}": v for i in range(LAYERS - 1) for k, v in list(wd.items())[:3]})
    wd["loss_reid"] = 2.0                       # meta_architecture.py from_config with MODEL.REFINER.USE_CL
    arrays = {"in/instance_embeds": instance.numpy(), "in/frame_embeds": frame.numpy(), "in/mask_features": mask_features.numpy(),
              "in/tgt_masks": tgt_masks.numpy().astype(np.uint8), "in/tgt_labels": labels.numpy()}
    meta = {"hidden": HID, "heads": HEADS, "ffn": FFN, "layers": LAYERS, "classes": NCLS, "T": T, "Q": Q, "H": H, "W": W, "G": G,
            "K": K, "weights": WEIGHTS, "weight_dict": wd, "weight_seed": seed, "max_len": MAX_LEN, "lr": LR, "steps": {}}
    torch.manual_seed(seed)
    ref = ref_mod.TemporalRefiner(hidden_channel=HID, feedforward_channel=FFN, num_head=HEADS, decoder_layer_num=LAYERS,
                                  mask_dim=HID, class_num=NCLS)
    with torch.no_grad():           # biases and norms away from their 0 / 1 initial values: their gradients then test something
        for n, p in ref.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape))
    ref.train()
    np.savez_compressed(OUT.format("_state"), **{k: v.numpy().copy() for k, v in ref.state_dict().items()})
    memory = utils_mod.Outputs_Memory_PerClasses(max_len=MAX_LEN)
    owner = types.SimpleNamespace(classes_references_memory=memory)
    matcher = vm.VideoHungarianMatcher(num_points=K * T, **WEIGHTS)
    crit = vc.VideoSetCriterion(NCLS, matcher=matcher, weight_dict=wd, eos_coef=0.1, losses=["labels", "masks"], num_points=K * T,
                                oversample_ratio=3.0, importance_sample_ratio=0.75)
    random.seed(16)
    for step in range(1, STEPS + 1):
        put = lambda name, v: arrays.__setitem__(f"step{step}/{name}", v.detach().numpy() if torch.is_tensor(v) else np.asarray(v))
        ref.zero_grad()
        out = ref(instance, frame, mask_features)
        for k in ("pred_logits", "pred_masks", "pred_embds"):
            put(k, out[k])
        for i, a in enumerate(out["aux_outputs"]):
            put(f"aux{i}/pred_logits", a["pred_logits"])
            put(f"aux{i}/pred_masks", a["pred_masks"])
        o2, targets = loss_reshape(out, tgt_masks, labels)
        torch.manual_seed(16 + step)
        with G14.Recorder() as crec:
            losses, match = crit(o2, targets, matcher_outputs=None, ret_match_result=True)
        had = {c: len(v) for c, v in memory.class_references.items()}
        with ShuffleRecorder() as srec:
            cl = meta_mod.DVIS_Plus_offline.get_cl_loss_with_memory(owner, o2, match, targets)
        losses.update(cl)
        assert set(losses) == set(wd) | {"loss_aux_reid"}, (sorted(losses), sorted(wd))
        assert float(losses["loss_reid"]) > 0 and len(srec.draws) >= 1
        assert all(len(v) <= MAX_LEN for v in memory.class_references.values())
        if step == 2:
            assert had, "step 2 must meet a filled memory (class items)"
        for i, d in enumerate(crec.draws):
            put(f"crit_draw_{i:02d}", d)
        for i, d in enumerate(srec.draws):
            put(f"shuffle_{i:02d}", d)
        put("match_idx", torch.stack(match[0]))
        for k, v in losses.items():
            put(f"loss/{k}", v)
        for c, rows in memory.class_references.items():
            put(f"memory/{c}", torch.stack(rows))
        sum(losses[k] * wd[k] for k in losses if k in wd).backward()
        grads = {}
        for n, p in ref.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
            grads[n] = p.grad.numpy().copy()
        np.savez_compressed(OUT.format(f"_grads_{step}"), **grads)
        with torch.no_grad():
            for p in ref.parameters():
                p.sub_(LR * p.grad)
        meta["steps"][step] = {"n_crit_draws": len(crec.draws), "n_shuffles": len(srec.draws), "loss_keys": sorted(losses),
                               "memory_before": had, "memory_after": {c: len(v) for c, v in memory.class_references.items()}}
        print("step", step, "match", [m.tolist() for m in match[0]], "memory", meta["steps"][step]["memory_after"],
              {k: round(float(v), 4) for k, v in losses.items()})
    arrays["meta"] = np.array(repr(meta))
    np.savez_compressed(OUT.format(""), **arrays)
    for suffix in ("", "_state", "_grads_1", "_grads_2"):
        print("wrote", OUT.format(suffix), os.path.getsize(OUT.format(suffix)), "bytes")
    print(len(spy.costs), "assignments stable at sigma 5e-3")


if __name__ == "__main__":
    main()
