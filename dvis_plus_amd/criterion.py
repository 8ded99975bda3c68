"""Set-prediction criterion of Mask2Former / DVIS++ with the reference's names, constructor arguments and loss-dict contract
(mask2former_video/modeling/criterion.py: VideoSetCriterion; mask2former/modeling/criterion.py: SetCriterion), and
``build_criterion(cfg, meta_arch)`` = the criterion part of the reference's three ``from_config``s.

``loss_masks`` runs on the fused HIP kernels for GPU tensors (functions.point_sample for the oversampling pass, torch.topk,
functions.point_mask_losses forward + backward) and on the torch formulations of cpu_ops.py for CPU tensors; ``loss_labels`` is
torch's cross_entropy ((B, Q, C + 1): not a hot path).  Half / bf16 mask logits are upcast to fp32 BEFORE sampling (the reference
samples in half and upcasts after).  Every random draw goes through ``_rand`` in the reference's order and shapes:
(R, int(num_points * oversample_ratio), 2) then (R, num_points - int(importance_sample_ratio * num_points), 2) per loss_masks.
"""
import random

import torch
import torch.nn.functional as F
from torch import nn

from . import functions as Fn
from .d2 import configurable
from .registry import Registry
from .matcher import HungarianMatcher, VideoHungarianMatcher, VideoHungarianMatcher_Consistent


def _world_size():
    d = torch.distributed
    return d.get_world_size() if d.is_available() and d.is_initialized() else 1


class VideoSetCriterion(nn.Module):
    """1) Hungarian assignment between the targets and the outputs, 2) classification and mask losses of the matched pairs.
    outputs: "pred_logits" (B, Q, C + 1), "pred_masks" (B, Q, T, H, W), optionally "aux_outputs": a list of such dicts.
    targets[b]: "labels" (G), "masks" (G, T, H, W)."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses, num_points, oversample_ratio,
                 importance_sample_ratio, frames=2):
        super().__init__()
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.eos_coef = eos_coef
        self.losses = losses
        empty_weight = torch.ones(self.num_classes + 1)
        empty_weight[-1] = self.eos_coef
        self.register_buffer("empty_weight", empty_weight)
        self.num_points = num_points
        self.oversample_ratio = oversample_ratio
        self.importance_sample_ratio = importance_sample_ratio
        self.frames = frames

    def _rand(self, shape, device):
        """Every random draw of the criterion: override to replay recorded draws."""
        return torch.rand(shape, device=device)

    def loss_labels(self, outputs, targets, indices, num_masks):
        logits = outputs["pred_logits"].float()
        idx = self._get_src_permutation_idx(indices)
        matched = torch.cat([t["labels"][J.to(t["labels"].device)] for t, (_, J) in zip(targets, indices)])
        classes = torch.full(logits.shape[:2], self.num_classes, dtype=torch.int64, device=logits.device)
        classes[idx] = matched.to(classes)
        return {"loss_ce": F.cross_entropy(logits.transpose(1, 2), classes, self.empty_weight)}

    def _matched_rows(self, outputs, targets, indices):
        """(src rows (R, H, W), target rows (R, H, W)) of the matched pairs, frames flattened into rows."""
        src = outputs["pred_masks"][self._get_src_permutation_idx(indices)]
        tgt = torch.cat([t["masks"][J.to(t["masks"].device)] for t, (_, J) in zip(targets, indices)])
        return src.flatten(0, 1), tgt.flatten(0, 1)

    def uncertain_point_coords(self, src_rows):
        """detectron2's get_uncertain_point_coords_with_randomness with uncertainty -|logit|: of int(num_points * oversample_ratio)
        uniform points per row keep the int(importance_sample_ratio * num_points) most uncertain, fill up with uniform points."""
        R, dev = src_rows.shape[0], src_rows.device
        n_sampled = int(self.num_points * self.oversample_ratio)
        n_uncertain = int(self.importance_sample_ratio * self.num_points)
        n_random = self.num_points - n_uncertain
        coords = self._rand((R, n_sampled, 2), dev)
        uncertainty = -Fn.point_sample(src_rows, coords).abs()
        idx = torch.topk(uncertainty, k=n_uncertain, dim=1)[1]
        picked = torch.gather(coords, 1, idx[:, :, None].expand(R, n_uncertain, 2))
        if n_random > 0:
            picked = torch.cat([picked, self._rand((R, n_random, 2), dev)], dim=1)
        return picked

    def loss_masks(self, outputs, targets, indices, num_masks):
        src_rows, tgt_rows = self._matched_rows(outputs, targets, indices)
        with torch.no_grad():
            coords = self.uncertain_point_coords(src_rows)
        loss_mask, loss_dice = Fn.point_mask_losses(src_rows, tgt_rows.to(src_rows.device), coords, num_masks)
        return {"loss_mask": loss_mask, "loss_dice": loss_dice}

    def _get_src_permutation_idx(self, indices):
        batch_idx = torch.cat([torch.full_like(src, i) for i, (src, _) in enumerate(indices)])
        return batch_idx, torch.cat([src for (src, _) in indices])

    def _get_tgt_permutation_idx(self, indices):
        batch_idx = torch.cat([torch.full_like(tgt, i) for i, (_, tgt) in enumerate(indices)])
        return batch_idx, torch.cat([tgt for (_, tgt) in indices])

    def get_loss(self, loss, outputs, targets, indices, num_masks):
        loss_map = {"labels": self.loss_labels, "masks": self.loss_masks}
        assert loss in loss_map, f"do you really want to compute {loss} loss?"
        return loss_map[loss](outputs, targets, indices, num_masks)

    def forward(self, outputs, targets, matcher_outputs=None, ret_match_result=False):
        """-> dict of losses ("loss_ce", "loss_mask", "loss_dice" and their "_i" copies per aux_outputs entry) [, indices].
        matcher_outputs: match on these outputs instead (once; the aux layers then reuse the pairs)."""
        matched_on = outputs if matcher_outputs is None else matcher_outputs
        indices = self.matcher({k: v for k, v in matched_on.items() if k != "aux_outputs"}, targets)
        num_masks = torch.as_tensor([sum(len(t["labels"]) for t in targets)], dtype=torch.float,
                                    device=next(iter(outputs.values())).device)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(num_masks)
        num_masks = torch.clamp(num_masks / _world_size(), min=1).item()

        losses = {}
        for loss in self.losses:
            losses.update(self.get_loss(loss, outputs, targets, indices, num_masks))
        for i, aux in enumerate(outputs.get("aux_outputs", ())):
            if matcher_outputs is None:
                indices = self.matcher(aux, targets)
            for loss in self.losses:
                losses.update({f"{k}_{i}": v for k, v in self.get_loss(loss, aux, targets, indices, num_masks).items()})
        return (losses, indices) if ret_match_result else losses

    def __repr__(self):
        body = [f"matcher: {self.matcher.__repr__(_repr_indent=8)}"] + [
            f"{k}: {getattr(self, k)}" for k in ("losses", "weight_dict", "num_classes", "eos_coef", "num_points",
                                                  "oversample_ratio", "importance_sample_ratio")]
        return "\n".join(["Criterion " + self.__class__.__name__] + [" " * 4 + line for line in body])


class SetCriterion(VideoSetCriterion):
    """The image model's criterion: "pred_masks" (B, Q, H, W), targets[b]["masks"] (G_b, H_b, W_b), zero-padded to one size."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses, num_points, oversample_ratio,
                 importance_sample_ratio):
        super().__init__(num_classes, matcher, weight_dict, eos_coef, losses, num_points, oversample_ratio,
                         importance_sample_ratio)
        del self.frames

    def _matched_rows(self, outputs, targets, indices):
        src = outputs["pred_masks"][self._get_src_permutation_idx(indices)]
        H = max(t["masks"].shape[-2] for t in targets)
        W = max(t["masks"].shape[-1] for t in targets)
        rows = []
        for t, (_, J) in zip(targets, indices):
            m = t["masks"][J.to(t["masks"].device)]
            rows.append(F.pad(m, (0, W - m.shape[-1], 0, H - m.shape[-2])))
        return src, torch.cat(rows)

    def forward(self, outputs, targets):
        return super().forward(outputs, targets)


def reference_contrastive_loss(references, match_result):
    """DVIS_Plus_online.get_cl_loss_ref + loss_reid (dvis_Plus/meta_architecture.py:981-1065, dvis_Plus/utils.py:51-94) in one
    batched form.  references (T, Q, C): the tracker's "pred_references", one row of queries per frame; match_result[t] = (query
    rows, target rows) of frame t.  Every matched query r of a frame t >= 1 is an anchor, once against frame t - 1 and, where
    there is one, once against frame t + 1: row r of that frame is its positive, the other Q - 1 rows are negatives.
    loss_reid = mean over the items of log(1 + sum_neg exp(neg . anchor - pos . anchor)); loss_aux_reid = mean over the items of
    mean_q (cos(row q, anchor) - [q == r])^2.  No item: both are 0 with a graph to `references`."""
    T, Q, _ = references.shape
    anchor_t, other_t, rows = [], [], []
    for t in range(1, T):
        src, tgt = match_result[t]
        by_target = {}
        for r, g in zip(src.tolist(), tgt.tolist()):
            by_target[g] = r
        for r in by_target.values():
            for o in (t - 1, t + 1):
                if o < T:
                    anchor_t.append(t), other_t.append(o), rows.append(r)
    if not rows:
        zero = references.sum() * 0
        return {"loss_reid": zero, "loss_aux_reid": zero}
    dev = references.device
    rows = torch.tensor(rows, device=dev)
    anchor = references[torch.tensor(anchor_t, device=dev), rows]                  # (n, C)
    other = references[torch.tensor(other_t, device=dev)]                          # (n, Q, C)
    dot = torch.einsum("nqc,nc->nq", other, anchor)
    # the positive's own entry is exactly 0: the "1 +" of the formula
    reid = torch.logsumexp(dot - dot.gather(1, rows[:, None]), dim=1).mean()
    cos = torch.einsum("nqc,nc->nq", F.normalize(other, dim=2), F.normalize(anchor, dim=1))
    aux = (cos - F.one_hot(rows, Q).to(cos.dtype)).square().mean()
    return {"loss_reid": reid, "loss_aux_reid": aux}


class Outputs_Memory_PerClasses:
    """The refiner stage's class-reference memory (dvis_Plus/utils.py:4-49, the part DVIS_Plus_offline uses): per class a list of
    embedding rows of earlier clips, detached, the negatives of ``refiner_contrastive_loss``'s class items.  A class that grows
    past ``max_len`` rows is shuffled and cut to its last ``max_len``; the shuffle is the memory's one random draw and goes through
    ``_draw`` so that recorded draws can be replayed."""

    def __init__(self, max_len=100):
        self.class_references = {}
        self.max_len = max_len

    def _draw(self, kind, n):
        """"shuffle", n -> a shuffled list(range(n)) (random.shuffle)."""
        if kind != "shuffle":
            raise ValueError(kind)
        indices = list(range(n))
        random.shuffle(indices)
        return indices

    def push_refiner(self, references, targets, match_result):
        """references (T, Q, C); targets: the video's target dict ("labels"); match_result (query rows, target rows): every matched
        query's T rows join its target's class."""
        references = references.clone().detach()
        classes = targets["labels"]
        for r, g in zip(match_result[0].tolist(), match_result[1].tolist()):
            self.class_references.setdefault(int(classes[g]), []).extend(torch.unbind(references[:, r], dim=0))
        for cls, rows in self.class_references.items():
            if len(rows) > self.max_len:
                order = self._draw("shuffle", len(rows))
                self.class_references[cls] = [rows[i] for i in order][-self.max_len:]

    def get_items(self, cls):
        rows = self.class_references.get(cls)
        return torch.stack(rows, dim=0) if rows else []


def refiner_contrastive_loss(pred_embds, match, labels, memory):
    """DVIS_Plus_offline.get_cl_loss_with_memory + loss_reid (dvis_Plus/meta_architecture.py:1502-1579, dvis_Plus/utils.py:51-94) in
    a batched form.  pred_embds (T, Q, C): the refiner's "pred_embds", one row of queries per frame; match = (query rows, target
    rows) of the video; labels (G) the targets' classes; memory: an Outputs_Memory_PerClasses.
    For every frame t and matched (query r, target g) one instance item: anchor = row r of frame t, positives = row r of all T
    frames (t included), negatives = the other Q - 1 rows of frame t; and, where the memory holds rows of g's class, one class
    item with the same anchor and positives and the memory's rows as negatives.
    loss_reid = mean over the items of logsumexp over all (negative - positive) . anchor pairs and one 0; loss_aux_reid = mean
    over the items of the mean squared difference between cosine and label (1 positive, 0 negative).  The clip's matched rows are
    then pushed into the memory.  No matched pair: both are 0 with a graph to `pred_embds`."""
    T, Q, C = pred_embds.shape
    by_target = {}
    for r, g in zip(match[0].tolist(), match[1].tolist()):
        by_target[g] = r
    reid, aux = [], []
    unit = F.normalize(pred_embds, dim=2)
    for g, r in by_target.items():
        anchor, u_anchor = pred_embds[:, r], unit[:, r]                            # (T, C): one anchor per frame
        pos = anchor @ anchor.t()                                                  # (T anchors, T positives)
        cos_pos = u_anchor @ u_anchor.t()
        others = [q for q in range(Q) if q != r]
        negatives = [(torch.einsum("tqc,tc->tq", pred_embds[:, others], anchor),
                      torch.einsum("tqc,tc->tq", unit[:, others], u_anchor))]
        rows = memory.get_items(int(labels[g]))
        if len(rows):
            rows = rows.to(pred_embds)
            negatives.append((anchor @ rows.t(), u_anchor @ F.normalize(rows, dim=1).t()))
        for neg, cos_neg in negatives:                                            # (T, N) each
            pairs = (neg[:, None, :] - pos[:, :, None]).flatten(1)                 # (T, T * N)
            reid.append(torch.logsumexp(F.pad(pairs, (0, 1)), dim=1))
            aux.append(((cos_pos - 1).square().sum(1) + cos_neg.square().sum(1)) / (T + neg.shape[1]))
    memory.push_refiner(pred_embds, {"labels": labels}, match)
    if not reid:
        zero = pred_embds.sum() * 0
        return {"loss_reid": zero, "loss_aux_reid": zero}
    return {"loss_reid": torch.cat(reid).mean(), "loss_aux_reid": torch.cat(aux).mean()}


class CTCLPlugin(nn.Module):
    """CTVIS's contrastive plugin on the segmenter's "pred_reid_embed" (dvis_Plus/ctvis.py:604-799 with its train memory :451-601
    and loss_reid :817-861): constructor arguments, ``from_config`` keys and ``weight_dict`` are the reference's.

    The reference keeps a memory bank of tensor slices per video and runs ~15 tiny ops per item; here ``train_loss`` does the
    bank's bookkeeping on indices and hands ALL items of the batch to ``Fn.contrastive_items`` in one call.  Per video and instance:
      * frame f, instance valid: its negatives of f = ``num_negatives`` rows sampled from ``range(num_negatives + 1)`` minus its
        matched query, sorted (the population is NOT range(Q): restated as written; num_negatives + 1 > Q raises); absent: all Q
        rows of f;
      * an item per frame f >= 1 where the instance is valid: anchor = its matched row of f, negatives = those of frame f - 1;
        positive = if the instance is valid somewhere before f: the similarity-guided embedding at f - 1 when ``momentum_embed`` and
        the coin ``np.random.rand() > 0.5`` say so, else its last valid row before f; if it is valid nowhere before f: its first valid
        row after f — but only when f differs from the NUMBER OF ABSENT frames after f (ctvis.py:518-519 compares these two;
        restated as written), else the item has no positive and is skipped.
    Similarity-guided embedding (:487-513): sg_1 = e_1, sg_k = (1 - beta_k) sg_(k-1) + beta_k e_k over the valid frames, beta_k =
    max(0, mean_(m < k) cos(e_m, e_k)), carried over absent frames; computed in torch for all instances at once (clamp(min=0): the
    value and gradient of the reference's python max except at exactly 0, without its host sync) and appended to the rows the
    kernel reads, so autograd carries the kernel's gradient back to "pred_reid_embed" through both.
    Every random draw goes through ``_draw`` in the reference's order.  Host syncs: the matcher's, and one copy of the ids."""

    @configurable
    def __init__(self, *, weight_dict, num_negatives, sampling_frame_num, bio_cl, momentum_embed, noise_embed):
        super().__init__()
        if noise_embed:
            raise NotImplementedError("CTCLPlugin: MODEL.CL_PLUGIN.NOISE_EMBED is not built (no config of the reference sets it)")
        self.weight_dict = weight_dict
        self.num_negatives = num_negatives
        self.sampling_frame_num = sampling_frame_num
        self.bio_cl = bio_cl
        self.momentum_embed = momentum_embed
        self.noise_embed = noise_embed
        self.last_items = None            # tests: the item table of the last train_loss call

    @classmethod
    def from_config(cls, cfg):
        cl = cfg.MODEL.CL_PLUGIN
        return {"weight_dict": {"loss_reid": cl.REID_WEIGHT, "loss_aux_reid": cl.AUX_REID_WEIGHT},
                "num_negatives": cl.NUM_NEGATIVES, "sampling_frame_num": cfg.INPUT.SAMPLING_FRAME_NUM, "bio_cl": cl.BIO_CL,
                "momentum_embed": cl.MOMENTUM_EMBED, "noise_embed": cl.NOISE_EMBED}

    def _draw(self, kind, *args):
        """Every random draw of the plugin: override to replay recorded draws.
        "negatives", population (ascending list), k -> random.sample(population, k), one per valid (video, frame, instance);
        "momentum" -> np.random.rand(), one per item that has a valid frame before it, when momentum_embed is set."""
        if kind == "negatives":
            return random.sample(args[0], args[1])
        if kind == "momentum":
            import numpy as np
            return float(np.random.rand())
        raise ValueError(kind)

    def match_frames(self, det_outputs, gt_instances, matcher):
        """One matcher call per frame index over the b videos (entries i::T), in that order."""
        T = self.sampling_frame_num
        tensors = {k: v for k, v in det_outputs.items() if k not in ("aux_outputs", "interm_outputs") and torch.is_tensor(v)}
        return [matcher({k: v[i::T] for k, v in tensors.items()}, gt_instances[i::T]) for i in range(T)]

    def build_items(self, indices_list, valid, Q):
        """The memory bank as index bookkeeping.  indices_list[f][v] = the matcher's (query rows, target rows) of video v in frame
        f; valid[v] = (G_v, T) nested lists of bools -> (items, sg_rows): items = dicts with "video", "frame", "instance", "anchor"
        (row of the (b T Q) rows), "pos" (row, or the (slot, frame) of a similarity-guided embedding when "pos_sg"), "neg" (rows);
        sg_rows[slot] = (the T matched rows of the instance behind that slot, 0 where absent; its T valid flags)."""
        T, K = self.sampling_frame_num, self.num_negatives
        items, sg_slots, sg_rows = [], {}, []
        for v, val in enumerate(valid):
            G = len(val)
            query = []                                   # [f][g]: the query matched to instance g in frame f
            for f in range(T):
                src, tgt = (t.tolist() for t in indices_list[f][v])
                by_target = dict(zip(tgt, src))
                query.append([by_target.get(g) for g in range(G)])
                if any(val[g][f] and query[f][g] is None for g in range(G)):
                    raise ValueError(f"CTCLPlugin: the matcher left a valid instance of video {v}, frame {f} without a query")
            row = lambda f, q: (v * T + f) * Q + q
            negatives = [[None] * G for _ in range(T)]
            for f in range(T):
                for g in range(G):
                    if val[g][f]:
                        if K + 1 > Q:
                            raise ValueError(f"CTCLPlugin: NUM_NEGATIVES + 1 = {K + 1} exceeds the {Q} queries (the reference samples "
                                             "its negatives from range(NUM_NEGATIVES + 1))")
                        population = [q for q in range(K + 1) if q != query[f][g]]
                        negatives[f][g] = [row(f, q) for q in sorted(self._draw("negatives", population, K))]
                    else:
                        negatives[f][g] = [row(f, q) for q in range(Q)]
            for f in range(1, T):
                for g in range(G):
                    if not val[g][f]:
                        continue
                    before = [m for m in range(f) if val[g][m]]
                    pos, pos_sg = None, False
                    if before:
                        if self.momentum_embed and self._draw("momentum") > 0.5:
                            if (v, g) not in sg_slots:
                                sg_slots[v, g] = len(sg_rows)
                                sg_rows.append(([row(m, query[m][g]) if val[g][m] else 0 for m in range(T)], val[g]))
                            pos, pos_sg = (sg_slots[v, g], f - 1), True
                        else:
                            pos = row(before[-1], query[before[-1]][g])
                    elif f != sum(1 for m in range(f + 1, T) if not val[g][m]):       # ctvis.py:518-519, as written
                        after = [m for m in range(f + 1, T) if val[g][m]]
                        if after:
                            pos = row(after[0], query[after[0]][g])
                    if pos is None:
                        continue
                    items.append({"video": v, "frame": f, "instance": g, "anchor": row(f, query[f][g]), "pos": pos,
                                  "pos_sg": pos_sg, "neg": negatives[f - 1][g]})
        return items, sg_rows

    def similarity_guided(self, reid, rows, valid):
        """reid (b T Q, C); rows (I, T) int64 the instances' matched rows (any row where absent), valid (I, T) bool (both on
        reid's device) -> (I, T, C): the similarity-guided embedding after each frame (zeros before the first valid frame)."""
        I, T = rows.shape
        e = reid[rows]                                                                           # (I, T, C)
        u = F.normalize(e, dim=-1)
        cos = u @ u.transpose(1, 2)                                                              # [i, m, k]
        pair = (valid[:, :, None] & valid[:, None, :]).to(e.dtype) * torch.triu(torch.ones(T, T, dtype=e.dtype, device=e.device), 1)
        before = (valid.to(torch.int64).cumsum(1) - valid.to(torch.int64))                      # valid frames before k
        beta = ((cos * pair).sum(1) / before.clamp(min=1).to(e.dtype)).clamp(min=0)
        beta = torch.where(valid, torch.where(before == 0, torch.ones_like(beta), beta), torch.zeros_like(beta))
        sg, out = torch.zeros_like(e[:, 0]), []
        for k in range(T):
            b = beta[:, k, None]
            sg = (1 - b) * sg + b * e[:, k]
            out.append(sg)
        return torch.stack(out, dim=1)

    def get_reid_loss(self, reid, indices_list, gt_instances):
        """reid ((b T), Q, C), the per-frame matches and the (b T) per-frame targets -> {"loss_reid", "loss_aux_reid"} unweighted."""
        T = self.sampling_frame_num
        BT, Q, C = reid.shape
        b = BT // T
        dev = reid.device
        zero = lambda: {"loss_reid": reid.sum() * 0, "loss_aux_reid": reid.sum() * 0}
        G = [int(gt_instances[v * T]["ids"].shape[0]) for v in range(b)]
        if sum(G) == 0:
            self.last_items = []
            return zero()
        ids = torch.cat([gt_instances[v * T + f]["ids"].reshape(-1) for v in range(b) for f in range(T)]).tolist()      # the one copy
        valid, off = [], 0
        for v in range(b):
            frames = [ids[off + f * G[v]:off + (f + 1) * G[v]] for f in range(T)]
            off += T * G[v]
            valid.append([[frames[f][g] != -1 for f in range(T)] for g in range(G[v])])
        items, sg_rows = self.build_items(indices_list, valid, Q)
        self.last_items = items
        if not items:
            return zero()
        src = reid.reshape(BT * Q, C)
        if src.dtype != torch.float32 and src.is_cuda:
            src = src.float()
        if sg_rows:
            sg = self.similarity_guided(src, torch.tensor([r for r, _ in sg_rows], device=dev),
                                        torch.tensor([v for _, v in sg_rows], device=dev))
            src = torch.cat([src, sg.reshape(-1, C)], dim=0)
        n = len(items)
        pos = [BT * Q + it["pos"][0] * T + it["pos"][1] if it["pos_sg"] else it["pos"] for it in items]
        neg_ptr = [0]
        for it in items:
            neg_ptr.append(neg_ptr[-1] + len(it["neg"]))
        i32 = lambda x: torch.tensor(x, dtype=torch.int32)
        reid_i, aux_i = Fn.contrastive_items(src.contiguous(), i32([it["anchor"] for it in items]), torch.arange(n + 1, dtype=torch.int32),
                                             i32(pos), i32(neg_ptr), i32([r for it in items for r in it["neg"]]))
        return {"loss_reid": reid_i.sum() / n, "loss_aux_reid": aux_i.sum() / n}

    def train_loss(self, det_outputs, gt_instances, matcher):
        """det_outputs: "pred_logits" ((b T), Q, K + 1), "pred_masks" ((b T), Q, h, w), "pred_reid_embed" ((b T), Q, C);
        gt_instances: the (b T) per-frame targets ("labels", "ids" (G), "masks" (G, h, w)); matcher: the image matcher.
        -> the two weighted losses."""
        indices_list = self.match_frames(det_outputs, gt_instances, matcher)
        losses = self.get_reid_loss(det_outputs["pred_reid_embed"], indices_list, gt_instances)
        return {k: v * self.weight_dict[k] for k, v in losses.items() if k in self.weight_dict}


CL_PLUGIN_REGISTRY = Registry("CL_PLUGIN")
CL_PLUGIN_REGISTRY.register(CTCLPlugin)


def build_cl_plugin(cfg):
    """ctvis.py:447-449."""
    return CL_PLUGIN_REGISTRY.get(cfg.MODEL.CL_PLUGIN.CL_PLUGIN_NAME)(cfg)


def build_criterion(cfg, meta_arch=None):
    """The criterion the reference's ``from_config`` of `meta_arch` builds (MODEL.META_ARCHITECTURE when None): "MinVIS"
    (dvis_Plus/meta_architecture.py:105-138) and "CTMinVIS" (the same), "DVIS_Plus_online" (:516-571), "DVIS_Plus_offline" (:1175-1243), "MaskFormer"
    (mask2former/maskformer_model.py:100-162) — matcher class, weights, weight_dict with its deep-supervision copies, losses."""
    meta_arch = cfg.MODEL.META_ARCHITECTURE if meta_arch is None else meta_arch
    if not isinstance(meta_arch, str):
        meta_arch = getattr(meta_arch, "__name__", type(meta_arch).__name__)
    mf = cfg.MODEL.MASK_FORMER
    weights = {"cost_class": mf.CLASS_WEIGHT, "cost_mask": mf.MASK_WEIGHT, "cost_dice": mf.DICE_WEIGHT}
    num_points, use_cl = mf.TRAIN_NUM_POINTS, False
    if meta_arch in ("MinVIS", "CTMinVIS"):              # ctvis.py:105-155 builds MinVIS's criterion
        matcher = VideoHungarianMatcher(num_points=num_points, **weights)
    elif meta_arch == "DVIS_Plus_online":
        matcher = VideoHungarianMatcher_Consistent(num_points=num_points, frames=cfg.INPUT.SAMPLING_FRAME_NUM, **weights)
        use_cl = getattr(cfg.MODEL.TRACKER, "USE_CL", False)
    elif meta_arch == "DVIS_Plus_offline":
        # the T frames of a clip are flattened into one (T h, w) image there: T times the points
        num_points = num_points * cfg.INPUT.SAMPLING_FRAME_NUM
        matcher = VideoHungarianMatcher(num_points=num_points, **weights)
        use_cl = getattr(cfg.MODEL.REFINER, "USE_CL", False)
    elif meta_arch == "MaskFormer":
        matcher = HungarianMatcher(num_points=num_points, **weights)
    else:
        raise ValueError(f"build_criterion: no criterion recipe for META_ARCHITECTURE {meta_arch!r}")
    weight_dict = {"loss_ce": mf.CLASS_WEIGHT, "loss_mask": mf.MASK_WEIGHT, "loss_dice": mf.DICE_WEIGHT}
    if mf.DEEP_SUPERVISION:
        base = dict(weight_dict)
        for i in range(mf.DEC_LAYERS - 1):
            weight_dict.update({f"{k}_{i}": v for k, v in base.items()})
    if use_cl:
        weight_dict["loss_reid"] = 2
    cls = SetCriterion if meta_arch == "MaskFormer" else VideoSetCriterion
    return cls(cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES, matcher=matcher, weight_dict=weight_dict, eos_coef=mf.NO_OBJECT_WEIGHT,
               losses=["labels", "masks"], num_points=num_points, oversample_ratio=mf.OVERSAMPLE_RATIO,
               importance_sample_ratio=mf.IMPORTANCE_SAMPLE_RATIO)
