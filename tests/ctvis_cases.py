"""Shared helpers of the CTVIS tests (test_contrastive_items_cpu.py, test_contrastive_items_gpu.py, test_ctvis_train_cpu.py,
test_ctvis_train_gpu.py): the per-item composition of the reference's contrastive loss restated from torch ops (the op-level
reference, fp32 and fp64 on the CPU), the op's cases, a brute-force inversion of the index lists, the g20 fixture (the reference's
own CTCLPlugin.train_loss and CTMinVIS.post_processing, tests/golden/gen_ctvis_golden.py) with replay of its recorded draws, and
the CTMinVIS toy stage."""
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from criterion_cases import Replay
from segmenter_train_cases import MIN_SAMPLES                          # noqa: F401
from vit_adapter_train_cases import SMALL, check_4x                    # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------ the per-item composition (ctvis.py:753-769, 836-857)
def item_losses(anchor, pos, neg):
    """One item as the reference composes it: anchor (C), pos (P, C), neg (N, C) -> (reid, aux) 0-d.  reid: logsumexp over the
    P * N differences (negative dot - positive dot) and one appended 0; aux: mean over the P + N rows of (cosine - label)^2 with
    F.normalize's cosine."""
    dp, dn = pos @ anchor, neg @ anchor
    pairs = (dn[None, :] - dp[:, None]).reshape(-1)
    reid = torch.logsumexp(torch.cat([pairs, pairs.new_zeros(1)]), dim=0)
    ua = F.normalize(anchor, dim=0)
    cos = torch.cat([F.normalize(pos, dim=1) @ ua - 1, F.normalize(neg, dim=1) @ ua])
    return reid, cos.square().mean()


def composition(src, lists):
    """All items of `lists` = (anchor, pos_ptr, pos_idx, neg_ptr, neg_idx) one by one -> (reid (n), aux (n))."""
    anchor, pos_ptr, pos_idx, neg_ptr, neg_idx = (t.tolist() for t in lists)
    out = [item_losses(src[a], src[pos_idx[pos_ptr[i]:pos_ptr[i + 1]]], src[neg_idx[neg_ptr[i]:neg_ptr[i + 1]]])
           for i, a in enumerate(anchor)]
    if not out:
        return src.new_zeros(0), src.new_zeros(0)
    return torch.stack([r for r, _ in out]), torch.stack([a for _, a in out])


def composition_reference(src, lists, g_reid, g_aux, dtype):
    """CPU autograd of the composition in `dtype` -> {"reid", "aux", "grad_src"}."""
    x = src.detach().cpu().to(dtype).requires_grad_()
    reid, aux = composition(x, lists)
    (grad,) = torch.autograd.grad((reid * g_reid.to(dtype)).sum() + (aux * g_aux.to(dtype)).sum(), x)
    return {"reid": reid.detach(), "aux": aux.detach(), "grad_src": grad}


def brute_force_transpose(lists, R):
    """The transposed lists by plain loops: per row its (global slot, item) occurrences in (item, slot) order, and the items it anchors."""
    anchor, pos_ptr, pos_idx, neg_ptr, neg_idx = (t.tolist() for t in lists)
    occ, roles = [[] for _ in range(R)], [[] for _ in range(R)]
    for i, a in enumerate(anchor):
        roles[a].append(i)
        base = pos_ptr[i] + neg_ptr[i]
        rows = pos_idx[pos_ptr[i]:pos_ptr[i + 1]] + neg_idx[neg_ptr[i]:neg_ptr[i + 1]]
        for s, r in enumerate(rows):
            occ[r].append((base + s, i))
    return occ, roles


def make_lists(items):
    """[(anchor, [positives], [negatives]), ...] -> the five int32 CPU tensors."""
    pos_ptr, neg_ptr = [0], [0]
    for _, p, n in items:
        pos_ptr.append(pos_ptr[-1] + len(p))
        neg_ptr.append(neg_ptr[-1] + len(n))
    t = lambda x: torch.tensor(x, dtype=torch.int32)
    return (t([a for a, _, _ in items]), t(pos_ptr), t([r for _, p, _ in items for r in p]), t(neg_ptr),
            t([r for _, _, n in items for r in n]))


def random_items(g, n, R, p_range, n_range):
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    rows = lambda k: torch.randint(0, R, (k,), generator=g).tolist()
    return [(ri(0, R - 1), rows(ri(*p_range)), rows(ri(*n_range))) for _ in range(n)]


def tile():
    """The slots one workgroup pass of the kernel's per-item reductions covers (the kernel's own constant)."""
    from dvis_plus_amd import native
    return int(native.lib().dvis_contrastive_items_tile())


# name -> (C, R, items or a callable(generator) -> items)
def _cases():
    cases = {}
    for C in (4, 64, 256, 260):
        cases[f"C{C}"] = (C, 12, lambda g: random_items(g, 3, 12, (1, 1), (5, 5)))
    cases["n1"] = (64, 9, lambda g: random_items(g, 1, 9, (1, 1), (7, 7)))
    # 37 items over 50 rows: every row is drawn many times, within a list (duplicates) and across roles
    cases["n37"] = (64, 50, lambda g: random_items(g, 37, 50, (1, 3), (0, 9)))
    for N in (0, 1, 7, 99, 199, 200):
        cases[f"N{N}"] = (64, 210, lambda g, N=N: random_items(g, 2, 210, (1, 1), (N, N)))
    cases["P5N3"] = (64, 12, lambda g: random_items(g, 1, 12, (5, 5), (3, 3)))
    cases["over_tile"] = (8, 40, lambda g: random_items(g, 2, 40, (2, 2), (tile() + 3, tile() + 3)))
    # row 0: anchor and positive of item 0; row 2: twice a negative of item 0 and the anchor of item 1; row 0 again a negative of
    # item 1; rows 10, 11: referenced by nobody
    cases["planted"] = (64, 12, [(0, [0, 1], [2, 2, 3]), (2, [4], [5, 0]), (7, [8], [6, 9])])
    return cases


OP_CASES = _cases()


@functools.lru_cache(maxsize=None)
def op_case(name):
    """Seeded inputs of a case and its fp32 / fp64 CPU references, computed once and left unchanged."""
    C, R, items = OP_CASES[name]
    g = torch.Generator().manual_seed(2000 + sorted(OP_CASES).index(name))
    if callable(items):
        items = items(g)
    lists = make_lists(items)
    src = torch.randn(R, C, generator=g) * (0.5 if C >= 64 else 1.0)
    n = len(items)
    g_reid, g_aux = torch.randn(n, generator=g), torch.randn(n, generator=g)
    return dict(src=src, lists=lists, g_reid=g_reid, g_aux=g_aux, R=R, C=C, n=n,
                cpu32=composition_reference(src, lists, g_reid, g_aux, torch.float32),
                cpu64=composition_reference(src, lists, g_reid, g_aux, torch.float64))


@functools.lru_cache(maxsize=None)
def big_dots_case():
    """Dots of +-80 and +-1e3 with an anchor of norm 10: margins of 160 and 2000 (the loss is linear in the margin there: no
    overflow), and of -160 and -2000 (the loss and its gradient vanish)."""
    g = torch.Generator().manual_seed(2099)
    C = 8
    src = torch.randn(9, C, generator=g) * 0.1
    src[0] = 0
    src[0, 0] = 10.0                                      # the anchor
    for r, d in zip(range(1, 9), (8.0, -8.0, 100.0, -100.0, 8.0, -8.0, 100.0, -100.0)):
        src[r, 0] = d                                     # rows 1..4 positives, 5..8 negatives: dots 80, -80, 1e3, -1e3
        src[r, 1:] += 0.3 * abs(d)
    lists = make_lists([(0, [2], [5]), (0, [4], [7]), (0, [1], [6]), (0, [3], [8]), (0, [1, 2], [5, 6])])
    g_reid, g_aux = torch.randn(5, generator=g), torch.randn(5, generator=g)
    return dict(src=src, lists=lists, g_reid=g_reid, g_aux=g_aux, R=9, C=C, n=5,
                cpu32=composition_reference(src, lists, g_reid, g_aux, torch.float32),
                cpu64=composition_reference(src, lists, g_reid, g_aux, torch.float64))


# ---------------------------------------------------------------------------------------------------------------- g20
class ReplayDraws:
    """A CTCLPlugin._draw that hands back the recorded samples and coins in order and checks what is asked for."""

    def __init__(self, samples, coins):
        self.samples, self.coins, self.i, self.j = [list(s) for s in samples], list(coins), 0, 0

    def __call__(self, kind, *args):
        if kind == "negatives":
            population, k = args
            assert population == sorted(population) and len(set(population)) == len(population)
            s = self.samples[self.i]
            self.i += 1
            assert len(s) == k and set(s) <= set(population), (s, population)
            return s
        assert kind == "momentum", kind
        self.j += 1
        return self.coins[self.j - 1]

    def exhausted(self):
        return self.i == len(self.samples) and self.j == len(self.coins)


class G20:
    def __init__(self):
        self.z = np.load(os.path.join(GOLDEN, "g20_ctvis.npz"))
        self.meta = eval(str(self.z["meta"]))          # repr() of a plain dict written by gen_ctvis_golden.py

    def t(self, name):
        return torch.from_numpy(self.z[name].copy())

    def det_outputs(self, device="cpu", dtype=torch.float32):
        return {"pred_logits": self.t("in/pred_logits").to(device), "pred_masks": (self.t("in/pred_masks8").float() / 8).to(device),
                "pred_reid_embed": self.t("in/pred_reid_embed").to(device=device, dtype=dtype).requires_grad_(True)}

    def targets(self, device="cpu"):
        n = self.meta["B"] * self.meta["T"]
        return [{"labels": self.t(f"tgt/labels_{e}").to(device), "ids": self.t(f"tgt/ids_{e}").to(device),
                 "masks": self.t(f"tgt/masks_{e}").float().to(device)} for e in range(n)]

    def matcher(self):
        from dvis_plus_amd.matcher import HungarianMatcher
        m = HungarianMatcher(num_points=self.meta["points"], **self.meta["weights"])
        m._rand = Replay([self.t(f"draw/matcher_{i:02d}") for i in range(self.meta["n_matcher_draws"])])
        return m

    def plugin(self, replay=True, **kw):
        from dvis_plus_amd.criterion import CTCLPlugin
        args = dict(weight_dict=dict(self.meta["loss_weights"]), num_negatives=self.meta["num_negatives"],
                    sampling_frame_num=self.meta["T"], bio_cl=False, momentum_embed=True, noise_embed=False)
        args.update(kw)
        p = CTCLPlugin(**args)
        if replay:
            p._draw = ReplayDraws(self.z["draw/samples"].tolist(), self.z["draw/coins"].tolist())
        return p

    def matched(self):
        T, B = self.meta["T"], self.meta["B"]
        return [[self.t(f"match/f{f}_v{v}") for v in range(B)] for f in range(T)]

    def items(self):
        """The reference's item table as the plugin's `last_items` entries (without the similarity-guided slot numbers)."""
        T, Q = self.meta["T"], self.meta["Q"]
        out = []
        for video, frame, inst, aq, kind, pf, pq, *neg in self.z["items/table"].tolist():
            out.append({"video": video, "frame": frame, "instance": inst, "anchor": (video * T + frame) * Q + aq,
                        "pos_sg": bool(kind), "pos": pf if kind else (video * T + pf) * Q + pq,
                        "neg": [(video * T + frame - 1) * Q + q for q in neg if q >= 0]})
        return out

    def run(self, device="cpu", dtype=torch.float32):
        """The plugin on the fixture with the recorded draws -> (plugin, indices_list, {"loss_reid", "loss_aux_reid", "grad"})."""
        det, plugin, matcher = self.det_outputs(device, dtype), self.plugin(), self.matcher()
        indices = plugin.match_frames(det, self.targets(device), matcher)
        losses = plugin.get_reid_loss(det["pred_reid_embed"], indices, self.targets(device))
        losses = {k: v * plugin.weight_dict[k] for k, v in losses.items()}
        (losses["loss_reid"] + losses["loss_aux_reid"]).backward()
        assert plugin._draw.exhausted() and matcher._rand.i == self.meta["n_matcher_draws"]
        return plugin, indices, {"loss_reid": losses["loss_reid"].detach(), "loss_aux_reid": losses["loss_aux_reid"].detach(),
                                 "grad": det["pred_reid_embed"].grad}


def plain_items(items):
    """`last_items` without the slot numbers of the similarity-guided embeddings: their frame stays."""
    return [dict(it, pos=it["pos"][1] if it["pos_sg"] else it["pos"]) for it in items]


# ------------------------------------------------------------------------------------------------ the CTMinVIS toy stage
def ctvis_cfg():
    from dvis_plus_amd.config import get_default_cfg
    with open(os.path.join(GOLDEN, "cfg_CTVIS_R50.json")) as f:
        return get_default_cfg().merge(json.load(f))


def toy_cfg():
    """ytvis19/CTVIS_R50.yaml at the sizes of segmenter_train_cases.minvis_model (g10's head on the toy backbone, T = 2)."""
    import segmenter_train_cases as S
    from conftest import Golden
    from toy_backbone import ToyBackbone
    from dvis_plus_amd.registry import BACKBONE_REGISTRY
    if "build_toy_backbone" not in BACKBONE_REGISTRY:
        def build_toy_backbone(cfg, input_shape=None):
            return ToyBackbone()
        BACKBONE_REGISTRY.register(build_toy_backbone)
    c = Golden("g10_window_loop").meta["cfg"]
    return ctvis_cfg().merge({
        "MODEL": {"BACKBONE": {"NAME": "build_toy_backbone"},
                  "SEM_SEG_HEAD": {"NUM_CLASSES": c["K"], "CONVS_DIM": c["hidden"], "MASK_DIM": c["mask_dim"],
                                   "TRANSFORMER_ENC_LAYERS": c["enc_layers"]},
                  "MASK_FORMER": {"HIDDEN_DIM": c["hidden"], "NHEADS": c["nheads"], "DIM_FEEDFORWARD": c["dec_ffn"],
                                  "DEC_LAYERS": c["dec_layers"] + 1, "NUM_OBJECT_QUERIES": c["Q"], "REID_HIDDEN_DIM": c["hidden"],
                                  "TRAIN_NUM_POINTS": 64},
                  "CL_PLUGIN": {"NUM_NEGATIVES": c["Q"] - 1}},
        "INPUT": {"SAMPLING_FRAME_NUM": S.T}})


def ctminvis_model(device="cpu", seed=20):
    """The toy CTMinVIS built by from_config, seeded, the offset / attention-weight projections randomised as in minvis_model."""
    from dvis_plus_amd.meta_architecture import CTMinVIS
    torch.manual_seed(seed)
    m = CTMinVIS(toy_cfg())
    m.reference_outputs = False
    with torch.no_grad():
        for layer in m.sem_seg_head.pixel_decoder.transformer.encoder.layers:
            layer.self_attn.sampling_offsets.weight.normal_(0, 0.3)
            layer.self_attn.attention_weights.weight.normal_(0, 0.5)
            layer.self_attn.attention_weights.bias.normal_(0, 0.5)
    return m.eval().to(device)
