"""Hungarian matchers of the set criterion, with the reference's names, constructor arguments and ``forward(outputs, targets)``
contract (mask2former_video/modeling/matcher.py, mask2former/modeling/matcher.py): a list with one
``(int64 prediction indices, int64 target indices)`` pair of CPU tensors per batch element, in scipy's order.

The cost matrix comes from ``functions.match_cost`` (one fused HIP launch on GPU tensors instead of the reference's
grid_sample + binary_cross_entropy x 2 + einsum x 3 chain; the torch formulation of cpu_ops.py on CPU tensors), the assignment
from the library's own solver ``dvis_lsap_solve`` (scipy's permutation, ties included), after ONE device-to-host copy of C per
matching call as in the reference.  Random sample points are drawn through ``_rand`` in the reference's order and shapes, so a
test can replay recorded draws.
"""
import ctypes

import numpy as np
import torch
from torch import nn

from . import functions as Fn
from . import native


def linear_sum_assignment(cost):
    """scipy.optimize.linear_sum_assignment for a (nr, nc) cost matrix (tensor or array) -> (row_ind, col_ind) int64 arrays, rows
    ascending.  dvis_lsap_solve wants nr <= nc: a taller matrix is solved transposed and mapped back, which is what scipy does
    too, so ties fall the same way."""
    c = cost.detach().cpu().numpy() if torch.is_tensor(cost) else np.asarray(cost)
    c = np.ascontiguousarray(c, dtype=np.float64)
    if c.ndim != 2:
        raise ValueError("expected a matrix (2-D array)")
    nr, nc = c.shape
    if nr == 0 or nc == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    transposed = nr > nc
    if transposed:
        c = np.ascontiguousarray(c.T)
    out = np.empty(c.shape[0], dtype=np.int64)
    rc = native.lib().dvis_lsap_solve(c.ctypes.data_as(ctypes.c_void_p), c.shape[0], c.shape[1],
                                      out.ctypes.data_as(ctypes.c_void_p))
    native.check(rc, "dvis_lsap_solve")
    if not transposed:
        return np.arange(nr, dtype=np.int64), out
    order = np.argsort(out, kind="stable")
    return out[order], order.astype(np.int64)


def _pairs(indices):
    return [(torch.as_tensor(np.asarray(i, dtype=np.int64)), torch.as_tensor(np.asarray(j, dtype=np.int64)))
            for i, j in indices]


class VideoHungarianMatcher(nn.Module):
    """1-to-1 assignment between the queries and the targets of each batch element.  outputs: "pred_logits" (B, Q, C + 1),
    "pred_masks" (B, Q, T, H, W); targets[b]: "labels" (G), "masks" (G, T, H, W) float, uint8 or bool."""

    def __init__(self, cost_class: float = 1, cost_mask: float = 1, cost_dice: float = 1, num_points: int = 0):
        super().__init__()
        self.cost_class = cost_class
        self.cost_mask = cost_mask
        self.cost_dice = cost_dice
        assert cost_class != 0 or cost_mask != 0 or cost_dice != 0, "all costs cant be 0"
        self.num_points = num_points

    def _rand(self, shape, device):
        """Every random draw of the matcher: override to replay recorded draws."""
        return torch.rand(shape, device=device)

    def cost_matrix(self, logits, out_mask, tgt_mask, tgt_ids):
        """C (Q, G) of one batch element; draws the (1, num_points, 2) sample points."""
        coords = self._rand((1, self.num_points, 2), out_mask.device)
        return Fn.match_cost(out_mask, tgt_mask, coords, logits, tgt_ids, self.cost_class, self.cost_mask, self.cost_dice)

    @torch.no_grad()
    def memory_efficient_forward(self, outputs, targets):
        indices = []
        for b in range(outputs["pred_logits"].shape[0]):
            C = self.cost_matrix(outputs["pred_logits"][b], outputs["pred_masks"][b], targets[b]["masks"],
                                 targets[b]["labels"])
            indices.append(linear_sum_assignment(C))
        return _pairs(indices)

    @torch.no_grad()
    def forward(self, outputs, targets):
        return self.memory_efficient_forward(outputs, targets)

    def __repr__(self, _repr_indent=4):
        lines = ["Matcher " + self.__class__.__name__] + [
            " " * _repr_indent + f"{k}: {getattr(self, k)}" for k in ("cost_class", "cost_mask", "cost_dice")]
        return "\n".join(lines)


class HungarianMatcher(VideoHungarianMatcher):
    """The image model's matcher (T = 1): "pred_masks" (B, Q, H, W), targets[b]["masks"] (G, H, W)."""


class VideoHungarianMatcher_Consistent(VideoHungarianMatcher):
    """The online model's matcher: the batch holds `frames` consecutive frames per video, an object is matched once, in the first
    frame where it appears (targets[b]["ids"] (G, 1) != -1), a query matched in an earlier frame is not available again
    (its row is set to 1e6), and every frame of the video receives the same pairs."""

    def __init__(self, cost_class: float = 1, cost_mask: float = 1, cost_dice: float = 1, num_points: int = 0,
                 frames: int = 5):
        super().__init__(cost_class=cost_class, cost_mask=cost_mask, cost_dice=cost_dice, num_points=num_points)
        self.frames = frames

    @torch.no_grad()
    def memory_efficient_forward(self, outputs, targets):
        indices = []
        for v in range(outputs["pred_logits"].shape[0] // self.frames):
            first = {}                                   # object -> first frame it appears in (insertion-ordered)
            for f in range(self.frames):
                ids = targets[v * self.frames + f]["ids"]
                for obj in torch.nonzero(ids.squeeze(1) != -1).flatten().tolist():
                    first.setdefault(obj, f)
            by_frame = {}
            for obj, f in first.items():
                by_frame.setdefault(f, []).append(obj)
            used, matched = [], ([], [])
            for f in sorted(by_frame):
                b, objs = v * self.frames + f, by_frame[f]
                sel = torch.as_tensor(objs, dtype=torch.int64, device=targets[b]["masks"].device)
                C = self.cost_matrix(outputs["pred_logits"][b], outputs["pred_masks"][b], targets[b]["masks"][sel],
                                     targets[b]["labels"][sel.to(targets[b]["labels"].device)]).cpu()
                if used:
                    C[used, :] = 1e6
                rows, cols = linear_sum_assignment(C)
                used += rows.tolist()
                matched[0].extend(rows.tolist())
                matched[1].extend(np.asarray(objs)[cols].tolist())
            indices += [matched] * self.frames
        return _pairs(indices)
