"""Writes tests/golden/g20_ctvis.npz and tests/golden/cfg_CTVIS_R50.json from the reference's own CTVIS code
(dvis_Plus/ctvis.py: CTCLPlugin.train_loss with its train memory and loss_reid, CTMinVIS.post_processing; the image matcher of
mask2former/modeling/matcher.py) and its configs/dvis_Plus/ytvis19/CTVIS_R50.yaml.

    python tests/golden/gen_ctvis_golden.py

Build-machine only; nothing at test time imports this file.  The reference files are imported UNCHANGED through _ref_import with
the stubs of gen_criterion_golden.py (un-vendored detectron2 names only).  The reference hard-codes device='cuda' in
TrainTracklet.__init__ and CTCLPlugin.device: torch.zeros is wrapped while the plugin runs (a 'cuda' device becomes the CPU) and the
property is replaced on the imported class.  Recorded, in order: the matcher's torch.rand draws, every random.sample result (with
the check that a draw from the ASCENDING list gives the same sample: the reference draws from a set), every np.random.rand value;
the matched indices, the item table (read off the tensors the memory bank hands out, by value), both weighted losses and the
gradient to pred_reid_embed with the embeddings in fp32 and in fp64.

Fixture conditions, asserted while searching seeds from SEED0: every assignment (matcher and alignment chain) is unchanged when
its cost matrix is perturbed by Gaussian noise of sigma = 5e-3 (50 draws); no beta of the similarity-guided fusion within 1e-3 of
0; no momentum coin within 1e-3 of 0.5.
"""
import json
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_import as R                # noqa: E402
import gen_criterion_golden as GC      # noqa: E402
from gen_cfg_fixtures import resolve   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "g20_ctvis.npz")
OUT_CFG = os.path.join(HERE, "cfg_CTVIS_R50.json")
C, Q, NNEG, T, B, NCLS, H, W, POINTS = 64, 8, 7, 4, 2, 5, 24, 40, 64
WEIGHTS = dict(cost_class=2.0, cost_mask=5.0, cost_dice=5.0)
LOSS_WEIGHTS = {"loss_reid": 2.0, "loss_aux_reid": 3.0}
# valid[v][g][f]: a full track; one absent from a middle frame (all-Q negatives, carried sg); one absent from frame 0 (positive
# taken from after); a full track; one valid in a single frame (no positive: the item is skipped)
VALID = [[[1, 1, 1, 1], [1, 1, 0, 1], [0, 1, 1, 1]], [[1, 1, 1, 1], [0, 0, 1, 0]]]
SEED0 = 2000


class FixtureCondition(AssertionError):
    pass


def install():
    GC.install()

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
    return R.ref("dvis_Plus.ctvis")


def inputs(seed):
    """Structured per-frame predictions around box targets (as g14), and reid embeddings around one prototype per instance."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B * T, Q, NCLS + 1, generator=g)
    masks = torch.randn(B * T, Q, H, W, generator=g) * 3.0
    reid = torch.randn(B * T, Q, C, generator=g) * 0.35
    targets = []
    for v in range(B):
        G = len(VALID[v])
        boxes = GC.boxes(g, G, T, H, W)                                    # (G, T, H, W) uint8
        labels = torch.randint(0, NCLS, (G,), generator=g)
        proto = torch.randn(G, C, generator=g) * 0.35
        for f in range(T):
            e = v * T + f
            ids = torch.tensor([10 * v + k if VALID[v][k][f] else -1 for k in range(G)])
            m = boxes[:, f].float() * torch.tensor([float(VALID[v][k][f]) for k in range(G)])[:, None, None]
            owners = torch.randperm(Q, generator=g)[:G]
            for k, q in enumerate(owners.tolist()):
                masks[e, q] = (m[k] * 2 - 1) * 4.0 + torch.randn(H, W, generator=g) * 1.5
                logits[e, q, labels[k]] += 3.0
                reid[e, q] = reid[e, q] + proto[k] * (1.0 if k % 2 == 0 else -0.2 + 0.8 * (f % 2))
            targets.append({"labels": labels.clone(), "ids": ids, "masks": m.clone()})
    masks = torch.clamp(torch.round(masks * 8), -127, 127) / 8             # exact in fp32
    return logits, masks, reid, targets


class Spy:
    """Everything the run records, and the wrappers that record it."""

    def __init__(self, mod):
        self.mod = mod
        self.samples, self.coins, self.betas, self.calls, self.video = [], [], [], [], -1

    def sample(self, population, k):
        state = random.getstate()
        out = random.sample(population, k)
        random.setstate(state)
        again = random.sample(sorted(population), k)
        assert out == again, "random.sample of the set differs from the sample of the ascending list"
        self.samples.append(sorted(out))
        return out

    def rand(self):
        v = float(np.random.rand())
        if abs(v - 0.5) < 1e-3:
            raise FixtureCondition("momentum coin within 1e-3 of 0.5")
        self.coins.append(v)
        return v

    def __enter__(self):
        mod, spy = self.mod, self
        self.saved = (mod.random, mod.np, mod.SimpleTrainMemory.empty, mod.SimpleTrainMemory.get_training_samples,
                      mod.TrainTracklet.update, torch.zeros, mod.CTCLPlugin.device)
        mod.random = types.SimpleNamespace(sample=self.sample, randint=random.randint)
        mod.np = types.SimpleNamespace(random=types.SimpleNamespace(rand=self.rand))
        empty, get, update, zeros = self.saved[2:6]

        def empty_spy(bank):
            spy.video += 1
            return empty(bank)

        def get_spy(bank, instance_id, frame_id):
            n0 = len(spy.coins)
            out = get(bank, instance_id, frame_id)
            spy.calls.append((spy.video, frame_id, instance_id, spy.coins[n0] if len(spy.coins) > n0 else float("nan"), out))
            return out

        def update_spy(tracklet, positive_embed, negative_embed, frame_id=0):
            if positive_embed is not None and tracklet.exist_frames > 0:
                prev = torch.cat([e for e in tracklet.reid_embeds if e is not None], dim=0).double()
                beta = float((F.normalize(prev, dim=-1) @ F.normalize(positive_embed[0].double(), dim=-1)).mean())
                if abs(beta) < 1e-3:
                    raise FixtureCondition("beta within 1e-3 of 0")
                spy.betas.append(beta)
            return update(tracklet, positive_embed, negative_embed, frame_id)

        def zeros_cpu(*a, **k):
            if str(k.get("device", "cpu")).startswith("cuda"):
                k["device"] = "cpu"
            return zeros(*a, **k)

        mod.SimpleTrainMemory.empty, mod.SimpleTrainMemory.get_training_samples = empty_spy, get_spy
        mod.TrainTracklet.update = update_spy
        torch.zeros = zeros_cpu
        mod.CTCLPlugin.device = property(lambda plugin: torch.device("cpu"))
        return self

    def __exit__(self, *exc):
        mod = self.mod
        (mod.random, mod.np, mod.SimpleTrainMemory.empty, mod.SimpleTrainMemory.get_training_samples, mod.TrainTracklet.update,
         torch.zeros, mod.CTCLPlugin.device) = self.saved


def row_of(rows, x):
    """The index of the row of `rows` (n, C) that equals x (C) exactly."""
    hit = (rows == x[None]).all(-1).nonzero().flatten().tolist()
    assert len(hit) == 1, hit
    return hit[0]


def run_plugin(mod, matcher_mod, seed, dtype):
    logits, masks, reid, targets = inputs(seed)
    reid = reid.to(dtype).requires_grad_(True)
    plugin = mod.CTCLPlugin(weight_dict=dict(LOSS_WEIGHTS), num_negatives=NNEG, sampling_frame_num=T, bio_cl=False,
                            momentum_embed=True, noise_embed=False)
    matcher = matcher_mod.HungarianMatcher(num_points=POINTS, **WEIGHTS)
    matched = []
    inner = matcher.forward

    def forward(outputs, tg):
        idx = inner(outputs, tg)
        matched.append([torch.stack((i, j)) for i, j in idx])
        return idx
    matcher.forward = forward
    torch.manual_seed(seed), random.seed(seed), np.random.seed(seed)
    det = {"pred_logits": logits, "pred_masks": masks, "pred_reid_embed": reid}
    gts = [{k: v.clone() for k, v in t.items()} for t in targets]
    with Spy(mod) as spy, GC.Recorder() as rec:
        losses = plugin.train_loss(det, gts, matcher)
    (losses["loss_reid"] + losses["loss_aux_reid"]).backward()
    return dict(logits=logits, masks=masks, reid=reid, targets=targets, losses=losses, grad=reid.grad, spy=spy, draws=rec.draws,
                matched=matched)


def item_table(run):
    """(n, 7 + Q) int64: video, frame, instance, anchor query, positive kind (0 raw row, 1 similarity-guided), positive frame,
    positive query (-1 for kind 1), then the negatives' queries in frame - 1, padded with -1; and the coins (nan: none drawn)."""
    reid = run["reid"].detach()
    table, coins = [], []
    for video, frame, inst, coin, (anchor, positive, negative) in run["spy"].calls:
        if positive is None:
            continue
        rows = lambda f: reid[video * T + f]
        aq = row_of(rows(frame), anchor[0].detach())
        if coin == coin and coin > 0.5:
            kind, pf, pq = 1, frame - 1, -1
        else:
            kind = 0
            (pf, pq), = [(f, row_of(rows(f), positive[0].detach())) for f in range(T)
                         if (rows(f) == positive[0].detach()[None]).all(-1).any()]
        nq = [row_of(rows(frame - 1), x.detach()) for x in negative]
        table.append([video, frame, inst, aq, kind, pf, pq] + nq + [-1] * (Q - len(nq)))
        coins.append(coin)
    return np.asarray(table, dtype=np.int64), np.asarray(coins, dtype=np.float64)


def post_processing(mod, seed):
    """CTMinVIS.post_processing on a T = 4 clip: permuted, noisy reid embeddings; every assignment stable at sigma 5e-3."""
    K, Qp, Cp, h, w = 5, 10, 16, 10, 14
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(Cp, Qp, generator=g)
    reid = torch.stack([base[:, torch.randperm(Qp, generator=g)] + 0.25 * torch.randn(Cp, Qp, generator=g) for _ in range(T)], 1)[None]
    logits = torch.randn(1, T, Qp, K + 1, generator=g) * 2
    masks = torch.randn(1, Qp, T, h, w, generator=g) * 3
    spy = GC.CostSpy()
    perms = []

    def lsa(cost):
        out = spy(cost)
        perms.append(np.asarray(out[1]))
        return out
    saved, mod.linear_sum_assignment = mod.linear_sum_assignment, lsa
    try:
        stub = types.SimpleNamespace()
        stub.match_from_embds = types.MethodType(mod.CTMinVIS.match_from_embds, stub)
        out = mod.CTMinVIS.post_processing(stub, dict(pred_logits=logits.clone(), pred_masks=masks.clone(), pred_reid_embed=reid.clone()))
    finally:
        mod.linear_sum_assignment = saved
    return {"pp/in_logits": logits, "pp/in_masks": masks, "pp/in_reid": reid, "pp/logits": out["pred_logits"],
            "pp/masks": out["pred_masks"], "pp/perms": np.stack(perms)}, dict(K=K, Q=Qp, C=Cp, T=T)


def main():
    mod = install()
    im = R.ref("mask2former.modeling.matcher")
    for seed in range(SEED0, SEED0 + 200):
        cost_spy = GC.CostSpy()
        im.linear_sum_assignment = cost_spy
        try:
            r32 = run_plugin(mod, im, seed, torch.float32)
            r64 = run_plugin(mod, im, seed, torch.float64)
            pp, pp_meta = post_processing(mod, seed)
        except FixtureCondition as e:
            print("seed", seed, "rejected:", e)
            continue
        except AssertionError as e:
            if "fixture condition" not in str(e):
                raise
            print("seed", seed, "rejected:", e)
            continue
        break
    else:
        raise SystemExit("no seed meets the fixture conditions")
    table, coins = item_table(r32)
    table64, _ = item_table(r64)
    assert np.array_equal(table, table64) and r32["spy"].samples == r64["spy"].samples and r32["spy"].coins == r64["spy"].coins
    kinds = table[:, 4].tolist()
    assert 0 in kinds and 1 in kinds, "the fixture needs raw and similarity-guided positives"
    n_calls = len(r32["spy"].calls)
    assert n_calls - len(table) == 1, "exactly the single-frame instance's item is skipped"
    arrays = {"in/pred_logits": r32["logits"], "in/pred_masks8": (r32["masks"] * 8).to(torch.int8), "in/pred_reid_embed": r32["reid"].detach()}
    for e, t in enumerate(r32["targets"]):
        arrays[f"tgt/labels_{e}"], arrays[f"tgt/ids_{e}"], arrays[f"tgt/masks_{e}"] = t["labels"], t["ids"], t["masks"].to(torch.uint8)
    for i, d in enumerate(r32["draws"]):
        arrays[f"draw/matcher_{i:02d}"] = d
    arrays["draw/samples"] = np.asarray(r32["spy"].samples, dtype=np.int64)
    arrays["draw/coins"] = np.asarray(r32["spy"].coins, dtype=np.float64)
    for f, per_video in enumerate(r32["matched"]):
        for v, idx in enumerate(per_video):
            arrays[f"match/f{f}_v{v}"] = idx
    arrays["items/table"], arrays["items/coins"] = table, coins
    for tag, r in (("f32", r32), ("f64", r64)):
        arrays[f"{tag}/loss_reid"], arrays[f"{tag}/loss_aux_reid"] = r["losses"]["loss_reid"].detach(), r["losses"]["loss_aux_reid"].detach()
        arrays[f"{tag}/grad_pred_reid_embed"] = r["grad"]
    arrays.update(pp)
    meta = dict(seed=seed, C=C, Q=Q, num_negatives=NNEG, T=T, B=B, NCLS=NCLS, H=H, W=W, points=POINTS, weights=WEIGHTS,
                loss_weights=LOSS_WEIGHTS, valid=VALID, n_matcher_draws=len(r32["draws"]), betas=[round(b, 6) for b in r32["spy"].betas],
                pp=pp_meta)
    arrays = {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    arrays["meta"] = np.array(repr(meta))
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; seed", seed, "items", len(table), "kinds", kinds, "betas", meta["betas"])
    with open(OUT_CFG, "w") as f:
        json.dump(resolve(os.path.join(R.REF, "configs", "dvis_Plus", "ytvis19", "CTVIS_R50.yaml")), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT_CFG)


if __name__ == "__main__":
    main()
