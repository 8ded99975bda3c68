"""Shared helpers of test_criterion_cpu.py / test_criterion_gpu.py: the g14 fixture as module inputs, replay of recorded random
draws, and an fp64 / fp32 torch evaluation of the reference's op sequence (grid_sample -> bce / einsum / dice) for the
production-shape comparisons."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class G14:
    def __init__(self):
        self.z = np.load(os.path.join(GOLDEN, "g14_criterion.npz"))
        self.meta = eval(str(self.z["meta"]))      # repr() of a plain dict written by gen_criterion_golden.py

    def t(self, case, name):
        return torch.from_numpy(self.z[f"{case}/{name}"].copy())

    def outputs(self, case, device, layers=None, requires_grad=False):
        m = self.meta["cases"][case]
        image = m.get("image", False)
        n = 1 + m.get("n_aux", 0) if layers is None else layers

        def one(i):
            masks = self.t(case, f"masks8_{i}").float() / 8
            if image:
                masks = masks[:, :, 0]
            return {"pred_masks": masks.to(device), "pred_logits": self.t(case, f"logits_{i}").to(device)}
        out = one(0)
        if requires_grad:
            out["pred_masks"].requires_grad_(True)
        if n > 1:
            out["aux_outputs"] = [one(i) for i in range(1, n)]
        return out

    def targets(self, case, device, dtype=torch.uint8):
        m = self.meta["cases"][case]
        image = m.get("image", False)
        out = []
        b = 0
        while f"{case}/tgt_masks_{b}" in self.z.files:
            masks = self.t(case, f"tgt_masks_{b}")
            t = {"labels": self.t(case, f"tgt_labels_{b}").to(device), "masks": (masks[:, 0] if image else masks).to(device, dtype)}
            if f"{case}/tgt_ids_{b}" in self.z.files:
                t["ids"] = self.t(case, f"tgt_ids_{b}").to(device)
            out.append(t)
            b += 1
        return out


class Replay:
    """A `_rand` that hands back recorded draws in order and checks the requested shapes."""

    def __init__(self, draws):
        self.draws, self.i = list(draws), 0

    def __call__(self, shape, device):
        d = self.draws[self.i]
        self.i += 1
        assert tuple(d.shape) == tuple(shape), (self.i - 1, tuple(d.shape), tuple(shape))
        return d.to(device)


def sample(maps, coords, dtype):
    """(N, C, H, W) maps at coords (N, P, 2) -> (N, C, P), grid_sample as detectron2's point_sample calls it."""
    if maps.shape[0] == 0:
        return maps.new_zeros((0, maps.shape[1], coords.shape[1]), dtype=dtype)
    return F.grid_sample(maps.to(dtype), 2.0 * coords.to(dtype)[:, :, None, :] - 1.0, mode="bilinear", padding_mode="zeros",
                         align_corners=False)[..., 0]


def cost_terms_torch(pred, tgt, coords, logits, ids, dtype):
    """The reference's op sequence for (cost_class, cost_mask, cost_dice), matcher.py:107-151, in `dtype` on CPU tensors."""
    Q, G, K = pred.shape[0], tgt.shape[0], coords.shape[-2]
    c = coords.reshape(1, K, 2)
    x = sample(pred, c.repeat(Q, 1, 1), dtype).flatten(1)
    t = sample(tgt, c.repeat(G, 1, 1), dtype).flatten(1)
    pos = F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction="none")
    neg = F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")
    cost_mask = (torch.einsum("nc,mc->nm", pos, t) + torch.einsum("nc,mc->nm", neg, 1 - t)) / x.shape[1]
    s = x.sigmoid()
    cost_dice = 1 - (2 * torch.einsum("nc,mc->nm", s, t) + 1) / (s.sum(-1)[:, None] + t.sum(-1)[None, :] + 1)
    cost_class = -logits.to(dtype).softmax(-1)[:, ids]
    return cost_class, cost_mask, cost_dice


def point_losses_torch(src, tgt, coords, num_masks, dtype):
    """The reference's loss_masks tail (criterion.py:21-67) at given points, in `dtype`: (loss_mask, loss_dice)."""
    x = sample(src[:, None], coords, dtype)[:, 0]
    t = sample(tgt[:, None], coords, dtype)[:, 0]
    loss_mask = F.binary_cross_entropy_with_logits(x, t, reduction="none").mean(1).sum() / num_masks
    s = x.sigmoid()
    loss_dice = (1 - (2 * (s * t).sum(-1) + 1) / (s.sum(-1) + t.sum(-1) + 1)).sum() / num_masks
    return loss_mask, loss_dice


def structured(seed, Q, G, T, H, W, ncls=40):
    """Seeded structured inputs: box targets, G queries are noisy copies, the rest noise (the fixture condition's kind)."""
    g = torch.Generator().manual_seed(seed)
    tgt = torch.zeros(G, T, H, W, dtype=torch.uint8)
    for k in range(G):
        h, w = int(torch.randint(H // 5, H // 2, (1,), generator=g)), int(torch.randint(W // 5, W // 2, (1,), generator=g))
        y, x = int(torch.randint(0, H - h, (1,), generator=g)), int(torch.randint(0, W - w, (1,), generator=g))
        for t in range(T):
            dx = min(x + 3 * t, W - w)
            tgt[k, t, y:y + h, dx:dx + w] = 1
    pred = torch.randn(Q, T, H, W, generator=g) * 3
    owners = torch.randperm(Q, generator=g)[:G]
    labels = torch.randint(0, ncls, (G,), generator=g)
    logits = torch.randn(Q, ncls + 1, generator=g)
    for k, q in enumerate(owners.tolist()):
        pred[q] = (tgt[k].float() * 2 - 1) * 4 + torch.randn(T, H, W, generator=g) * 1.5
        logits[q, labels[k]] += 3
    return pred, tgt, labels, logits, owners
