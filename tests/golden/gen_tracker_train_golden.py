"""Writes tests/golden/g15_tracker_train.npz (+ g15_tracker_train_grads_{wa,cc,rs}.npz: one file per noise mode keeps every
file below the size limit) from the reference's own ReferringTracker_noiser in TRAINING mode (dvis_Plus/tracker.py,
dvis_Plus/noiser.py), its VideoSetCriterion with the consistent matcher (mask2former_video/modeling/{criterion,matcher}.py)
and DVIS_Plus_online.get_cl_loss_ref + loss_reid (dvis_Plus/meta_architecture.py, dvis_Plus/utils.py) on its output.

    python tests/golden/gen_tracker_train_golden.py

Build-machine only; nothing at test time imports this file.  The reference files are imported UNCHANGED through _ref_import.py
with the stubs of gen_criterion_golden.py.  The model's reshape between tracker and criterion
(DVIS_Plus_online.frame_decoder_loss_reshape: 'b q t h w -> (b t) q () h w', targets split per frame) is restated below with
torch ops.  Every random draw is recorded in order: random.random, np.random.shuffle, torch.rand and torch.randint
inside the tracker call (the noiser), torch.rand inside the criterion call (matcher and point sampling).

Setup: hidden 64, 2 heads, FFN 128, 2 layers, 5 classes, mask dim 64; T = 3, Q = 8, a 12 x 20 map, 3 ground-truth instances;
noise_ratio 1.0, once per noise mode 'wa', 'cc', 'rs' (the same weights and inputs).  Fixture condition, as in g14: every
assignment that is used (the matcher's, and the noiser's wherever its references are distinct rows) is unchanged when its cost matrix is perturbed by Gaussian noise of sigma 5e-3.
"""
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_import as R    # noqa: E402
import gen_criterion_golden as G14    # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "g15_tracker_train.npz")
HID, HEADS, FFN, LAYERS, NCLS, T, Q, H, W, G, K = 64, 2, 128, 2, 5, 3, 8, 12, 20, 3, 64
WEIGHTS = dict(cost_class=2.0, cost_mask=5.0, cost_dice=5.0)
MODES = ("wa", "cc", "rs")


class DrawRecorder:
    """random.random, np.random.shuffle, torch.rand, torch.randint replaced by recording wrappers while active."""

    def __init__(self):
        self.draws = []      # (kind, value)

    def __enter__(self):
        self._orig = (random.random, np.random.shuffle, torch.rand, torch.randint)
        o_random, o_shuffle, o_rand, o_randint = self._orig

        def rnd():
            v = o_random()
            self.draws.append(("random", np.float64(v)))
            return v

        def shuffle(x):
            o_shuffle(x)
            self.draws.append(("shuffle", np.array(x, dtype=np.int64)))

        def rand(*a, **k):
            v = o_rand(*a, **k)
            self.draws.append(("rand", v.clone().numpy()))
            return v

        def randint(*a, **k):
            v = o_randint(*a, **k)
            self.draws.append(("randint", v.clone().numpy()))
            return v
        random.random, np.random.shuffle, torch.rand, torch.randint = rnd, shuffle, rand, randint
        return self

    def __exit__(self, *exc):
        random.random, np.random.shuffle, torch.rand, torch.randint = self._orig


def inputs():
    gen = torch.Generator().manual_seed(1500)
    base = torch.randn(Q, HID, generator=gen)
    frames = []
    for t in range(T):
        perm = torch.randperm(Q, generator=gen)
        frames.append(base[perm] + 0.05 * torch.randn(Q, HID, generator=gen))
    fe_nn = torch.stack(frames)                                             # (t, q, c)
    fe = F.layer_norm(fe_nn, (HID,))
    to_bctq = lambda z: z.permute(2, 0, 1).unsqueeze(0).contiguous()
    mask_features = torch.randn(1, T, HID, H, W, generator=gen)
    tgt_masks = G14.boxes(gen, G, T, 2 * H, 2 * W).float()                  # (g, t, 24, 40)
    labels = torch.randint(0, NCLS, (G,), generator=gen)
    ids = torch.arange(G)[:, None].repeat(1, T)
    return to_bctq(fe), to_bctq(fe_nn), mask_features, tgt_masks, labels, ids


def loss_reshape(outputs, tgt_masks, labels, ids):
    def one(d):
        return {"pred_masks": d["pred_masks"].permute(0, 2, 1, 3, 4).flatten(0, 1).unsqueeze(2),
                "pred_logits": d["pred_logits"].flatten(0, 1)}
    out = one(outputs)
    out["aux_outputs"] = [one(a) for a in outputs["aux_outputs"]]
    targets = [{"labels": labels, "ids": ids[:, [f]], "masks": tgt_masks[:, [f]]} for f in range(T)]
    return out, targets


def ref_meta():
    """dvis_Plus.meta_architecture with the un-vendored detectron2 names it imports stubbed (as gen_criterion_golden.weight_dicts
    does); the reference's own criterion / matcher modules stay the real ones.  Only get_cl_loss_ref is used."""
    class _Any:
        def __init__(self, *a, **k):
            pass
    R._mod("detectron2.data", MetadataCatalog=_Any)
    dm = sys.modules["detectron2.modeling"]
    dm.build_backbone = dm.build_sem_seg_head = None
    R._mod("detectron2.modeling.backbone", Backbone=_Any)
    R._mod("detectron2.structures", Boxes=_Any, ImageList=_Any, Instances=_Any, BitMasks=_Any)
    m = types.ModuleType("mask2former_video.utils")
    m.__path__ = [f"{R.REF}/mask2former_video/utils"]
    sys.modules["mask2former_video.utils"] = m
    return R.ref("dvis_Plus.meta_architecture")


def main():
    """A randomly initialised tracker gives the matcher near-ties for most weight seeds: take the first seed from 1501 on at which
    the fixture condition holds for all three modes."""
    G14.install()
    for seed in range(1501, 1601):
        try:
            return generate(seed)
        except AssertionError as e:
            if "fixture condition" not in str(e):
                raise
            print("seed", seed, ":", e)
    raise SystemExit("no seed met the fixture condition")


def generate(seed):
    trk_mod = R.ref("dvis_Plus.tracker")
    noiser_mod = R.ref("dvis_Plus.noiser")
    vm = R.ref("mask2former_video.modeling.matcher")
    vc = R.ref("mask2former_video.modeling.criterion")
    meta_mod = ref_meta()
    spy = G14.CostSpy()
    vm.linear_sum_assignment = spy

    def noiser_lsa(C):
        # 'wa' / 'cc' return indices with repeats, so the next frame's references hold equal rows and its assignment has an exact
        # tie by construction — and is thrown away: at noise_ratio 1.0 the noiser returns its noised indices from frame 1 on.
        # The fixture condition applies to the assignments that are used (no equal rows).
        c = C.numpy() if torch.is_tensor(C) else np.asarray(C)
        if len(np.unique(c.round(6), axis=0)) < len(c):
            return spy.lsa(c)
        return spy(c)
    noiser_mod.linear_sum_assignment = noiser_lsa
    fe, fe_nn, mask_features, tgt_masks, labels, ids = inputs()
    wd = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    wd.update({f"{k}_{i}": v for i in range(LAYERS - 1) for k, v in list(wd.items())[:3]})
    wd["loss_reid"] = 2.0                       # meta_architecture.py from_config with MODEL.TRACKER.USE_CL
    arrays = {"in/frame_embeds": fe.numpy(), "in/frame_embeds_no_norm": fe_nn.numpy(), "in/mask_features": mask_features.numpy(),
              "in/tgt_masks": tgt_masks.numpy().astype(np.uint8), "in/tgt_labels": labels.numpy(), "in/tgt_ids": ids.numpy()}
    meta = {"hidden": HID, "heads": HEADS, "ffn": FFN, "layers": LAYERS, "classes": NCLS, "T": T, "Q": Q, "H": H, "W": W, "G": G,
            "K": K, "weights": WEIGHTS, "weight_dict": wd, "weight_seed": seed, "modes": {}}
    for mode in MODES:
        torch.manual_seed(seed)
        trk = trk_mod.ReferringTracker_noiser(hidden_channel=HID, feedforward_channel=FFN, num_head=HEADS,
                                              decoder_layer_num=LAYERS, mask_dim=HID, class_num=NCLS, noise_mode=mode,
                                              noise_ratio=1.0)
        with torch.no_grad():       # biases and norms away from their 0 / 1 initial values: their gradients then test something
            for n, p in trk.named_parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn(p.shape))
        trk.train()
        if mode == MODES[0]:
            for k, v in trk.state_dict().items():
                arrays[f"state/{k}"] = v.numpy().copy()
        noised = []
        orig_call = noiser_mod.Noiser.__call__

        def spy_call(self, *a, **k):
            idx, init = orig_call(self, *a, **k)
            noised.append(init.detach().clone())
            return idx, init
        noiser_mod.Noiser.__call__ = spy_call
        random.seed(15), np.random.seed(15), torch.manual_seed(15)
        try:
            with DrawRecorder() as rec:
                out, indices = trk(fe, mask_features, return_indices=True, frame_classes=None, frame_embeds_no_norm=fe_nn)
        finally:
            noiser_mod.Noiser.__call__ = orig_call
        put = lambda name, v: arrays.__setitem__(f"{mode}/{name}", v.detach().numpy() if torch.is_tensor(v) else np.asarray(v))
        for i, (kind, v) in enumerate(rec.draws):
            put(f"draw_{i:02d}_{kind}", v)
        put("indices", np.stack([np.asarray(ix, dtype=np.int64) for ix in indices]))
        put("noised_init", torch.stack(noised))
        for k in ("pred_logits", "pred_masks", "pred_embds", "pred_references"):
            put(k, out[k])
        for i, a in enumerate(out["aux_outputs"]):
            put(f"aux{i}/pred_logits", a["pred_logits"])
            put(f"aux{i}/pred_masks", a["pred_masks"])
        matcher = vm.VideoHungarianMatcher_Consistent(num_points=K, frames=T, **WEIGHTS)
        crit = vc.VideoSetCriterion(NCLS, matcher=matcher, weight_dict=wd, eos_coef=0.1, losses=["labels", "masks"], num_points=K,
                                    oversample_ratio=3.0, importance_sample_ratio=0.75)
        o2, targets = loss_reshape(out, tgt_masks, labels, ids)
        torch.manual_seed(16)
        with G14.Recorder() as crec:
            losses, match = crit(o2, targets, matcher_outputs=None, ret_match_result=True)
        # DVIS_Plus_online.forward under use_cl: the contrastive loss of the reference embeddings on the LAST match result;
        # loss_aux_reid is recorded and, not being in the weight_dict, dropped from the weighted sum as the reference drops it
        o2["pred_references"] = out["pred_references"].permute(0, 2, 3, 1).flatten(0, 1)         # 'b c t q -> (b t) q c'
        losses.update(meta_mod.DVIS_Plus_online.get_cl_loss_ref(None, o2, match))
        assert set(losses) == set(wd) | {"loss_aux_reid"}, (sorted(losses), sorted(wd))
        assert float(losses["loss_reid"]) > 0
        for i, d in enumerate(crec.draws):
            put(f"crit_draw_{i:02d}", d)
        for b, (i, j) in enumerate(match):
            put(f"match_idx_{b}", torch.stack((i, j)))
        for k, v in losses.items():
            put(f"loss/{k}", v)
        sum(losses[k] * wd[k] for k in losses if k in wd).backward()
        grads = {}
        for n, p in trk.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
            grads[n] = p.grad.numpy().copy()
        gpath = os.path.join(HERE, f"g15_tracker_train_grads_{mode}.npz")
        np.savez_compressed(gpath, **grads)
        meta["modes"][mode] = {"n_draws": len(rec.draws), "draw_kinds": [k for k, _ in rec.draws], "n_crit_draws": len(crec.draws),
                               "loss_keys": sorted(losses)}
        print(mode, "draws", [k for k, _ in rec.draws], "indices", [list(map(int, ix)) for ix in indices],
              "wrote", gpath, os.path.getsize(gpath), "bytes")
    arrays["meta"] = np.array(repr(meta))
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(spy.costs), "assignments stable at sigma 5e-3")


if __name__ == "__main__":
    main()
