"""Time CTVIS's contrastive plugin, forward + backward, on the contrastive-items kernel (csrc/contrastive_items.hip) against the
reference's per-item op sequence and against the batched torch formulation, and one CTMinVIS R50 training step with the kernel on
and off.

    python tools/ctvis_train_time.py [--repeats 5] [--iters 10] [--out profiles/ctvis_train_time.txt]

Every GPU step runs in a fresh child process under its own time limit; the first failure ends the run.  Steps:
  plugin b T Q    CTCLPlugin.get_reid_loss + backward on seeded embeddings (b videos, T = 10 frames, G = 6 instances, C = 256;
                  Q = 100 with NUM_NEGATIVES = 99: R50, Q = 200 with 199: ViT-Adapter-L).  One instance is absent from two middle
                  frames, one from frame 0.  The matcher is left out (the same on every side); the similarity-guided embeddings and
                  the host's index bookkeeping are in.  Three paths on the same items, alternated:
                    kernel     the plugin as shipped (Fn.contrastive_items, one forward launch, three backward launches)
                    batched    DVIS_CONTRASTIVE_ITEMS=0: cpu_ops.contrastive_items on the GPU
                    per_item   the reference's op sequence per item written out below (cat, einsum x 2, normalize x 2, the masked
                               pair matrix, pad, logsumexp, abs / pow / mean), without its two host syncs per item
                  Times are host clock around a call that ends in a device synchronise (the plugin is host-bound: device events
                  would miss the bookkeeping): median of --iters calls after 3 warm-up calls, --repeats times; `ms` = the median of
                  the repeats' medians, `spread` = max - min of them.  `launches` = GPU kernels of one forward + backward call,
                  counted by torch.profiler in a call of its own ("not measured" when the profiler reports none).
  step            one CTMinVIS training step (forward + backward, no optimizer), R50, b = 1, T = 10, 320 x 480, G = 6, kernel on
                  and off, alternated.
No GPU -> the tool fails (it never times a CPU)."""
import argparse
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
T, G, C = 10, 6, 256
STEPS = [("plugin", 1, 100), ("plugin", 8, 100), ("plugin", 1, 200), ("plugin", 8, 200), ("step", 1, 100)]
LIMIT = {"plugin": 240, "step": 420}


def wall(fn, iters, warmup=3):
    ts = []
    for i in range(iters + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and not e.name.startswith(("Memcpy", "Memset")))
    except Exception:
        return "not measured"
    return n if n else "not measured"


def with_env(value, fn):
    def run():
        prev = os.environ.get("DVIS_CONTRASTIVE_ITEMS")
        os.environ["DVIS_CONTRASTIVE_ITEMS"] = value
        try:
            return fn()
        finally:
            if prev is None:
                del os.environ["DVIS_CONTRASTIVE_ITEMS"]
            else:
                os.environ["DVIS_CONTRASTIVE_ITEMS"] = prev
    return run


def per_item_losses(src, items, BTQ, T_):
    """The reference's sequence, one item at a time (ctvis.py:753-769, 836-857), on rows of `src`."""
    contras, aux = 0, 0
    for it in items:
        anchor = src[it["anchor"]][None]
        pos = src[BTQ + it["pos"][0] * T_ + it["pos"][1]][None] if it["pos_sg"] else src[it["pos"]][None]
        rows = torch.cat([pos, src[it["neg"]]], dim=0)
        label = rows.new_zeros((rows.shape[0],), dtype=torch.int64)
        label[:1] = 1
        dot = torch.einsum("ac,kc->ak", rows, anchor)
        cos = torch.einsum("ac,kc->ak", F.normalize(rows, dim=1), F.normalize(anchor, dim=1))
        pred, lab = dot.permute(1, 0), label[None]
        is_pos, is_neg = lab == 1, lab == 0
        p, n = pred * is_pos.float(), pred * is_neg.float()
        p[is_neg] = p[is_neg] + float("inf")
        n[is_pos] = n[is_pos] + float("-inf")
        x = F.pad(n.repeat(1, pred.shape[1]) - torch.repeat_interleave(p, pred.shape[1], dim=1), (0, 1), "constant", 0)
        contras = contras + torch.logsumexp(x, dim=1)
        aux = aux + (torch.abs(cos.permute(1, 0) - lab) ** 2).mean()
    return contras.sum() / len(items), aux / len(items)


def plugin_step(b, Q, a):
    from dvis_plus_amd.criterion import CTCLPlugin
    g = torch.Generator().manual_seed(b * 1000 + Q)
    plugin = CTCLPlugin(weight_dict={"loss_reid": 2.0, "loss_aux_reid": 3.0}, num_negatives=Q - 1, sampling_frame_num=T, bio_cl=False,
                        momentum_embed=True, noise_embed=False)
    reid = (torch.randn(b * T, Q, C, generator=g) * 0.3).to(DEV).requires_grad_()
    indices = [[(torch.randperm(Q, generator=g)[:G], torch.arange(G)) for _ in range(b)] for _ in range(T)]
    ids = torch.arange(G).repeat(T, 1)                        # (T, G)
    ids[3:5, 5], ids[0, 4] = -1, -1
    gts = [{"ids": ids[f].to(DEV)} for _ in range(b) for f in range(T)]
    import random
    state = (random.getstate(), np.random.get_state())

    def seeded(fn):
        def run():
            random.setstate(state[0]), np.random.set_state(state[1])          # the same items on every path and call
            reid.grad = None
            return fn()
        return run

    def shipped():
        losses = plugin.get_reid_loss(reid, indices, gts)
        (2.0 * losses["loss_reid"] + 3.0 * losses["loss_aux_reid"]).backward()
        return losses

    def per_item():
        valid = [[[bool(ids[f, k] != -1) for f in range(T)] for k in range(G)] for _ in range(b)]
        items, sg_rows = plugin.build_items(indices, valid, Q)
        src = reid.reshape(b * T * Q, C)
        if sg_rows:
            sg = plugin.similarity_guided(src, torch.tensor([r for r, _ in sg_rows], device=DEV), torch.tensor([v for _, v in sg_rows], device=DEV))
            src = torch.cat([src, sg.reshape(-1, C)], dim=0)
        lr, la = per_item_losses(src, items, b * T * Q, T)
        (2.0 * lr + 3.0 * la).backward()
        return {"loss_reid": lr, "loss_aux_reid": la}
    paths = {"kernel": seeded(shipped), "batched": seeded(with_env("0", shipped)), "per_item": seeded(per_item)}
    ref, grads = {}, {}
    for name, fn in paths.items():
        out = fn()
        ref[name], grads[name] = {k: float(v.detach()) for k, v in out.items()}, reid.grad.clone()
    res = {k: [] for k in paths}
    for _ in range(a.repeats):
        for name, fn in paths.items():
            res[name].append(wall(fn, a.iters))
    line = {"step": "plugin fwd+bwd", "b": b, "T": T, "G": G, "Q": Q, "C": C, "items": len(plugin.last_items),
            "slots": sum(1 + len(it["neg"]) for it in plugin.last_items)}
    for name in paths:
        line[f"{name}_ms"] = round(float(np.median(res[name])), 3)
        line[f"{name}_spread_ms"] = round(max(res[name]) - min(res[name]), 3)
        line[f"{name}_launches"] = launches(paths[name])
    line["per_item_over_kernel"] = round(line["per_item_ms"] / line["kernel_ms"], 2)
    line["batched_over_kernel"] = round(line["batched_ms"] / line["kernel_ms"], 2)
    line["max_abs_grad_diff_vs_per_item"] = {k: float((grads[k] - grads["per_item"]).abs().max()) for k in ("kernel", "batched")}
    line["loss_reid"] = {k: round(v["loss_reid"], 6) for k, v in ref.items()}
    return line


def full_step(a):
    from dvis_plus_amd.config import build_model, get_default_cfg
    H, W = 320, 480
    cfg = get_default_cfg().merge({
        "MODEL": {"META_ARCHITECTURE": "CTMinVIS", "SEM_SEG_HEAD": {"NUM_CLASSES": 40},
                  "MASK_FORMER": {"CLASS_WEIGHT": 2.0, "MASK_WEIGHT": 5.0, "DICE_WEIGHT": 5.0, "NO_OBJECT_WEIGHT": 0.1,
                                  "DEEP_SUPERVISION": True, "TRAIN_NUM_POINTS": 12544, "OVERSAMPLE_RATIO": 3.0,
                                  "IMPORTANCE_SAMPLE_RATIO": 0.75}},
        "INPUT": {"SAMPLING_FRAME_NUM": T}})
    torch.manual_seed(0)
    m = build_model(cfg).to(DEV).train()
    g = torch.Generator().manual_seed(1)
    frames = [(torch.rand(3, H, W, generator=g) * 255).to(DEV) for _ in range(T)]
    instances = []
    for f in range(T):
        masks = torch.zeros(G, H, W, dtype=torch.bool)
        for k in range(G):
            masks[k, 20 + 40 * k:70 + 40 * k, 30 + 50 * k + 4 * f:120 + 50 * k + 4 * f] = True
        ids = torch.arange(G)
        if f in (3, 4):
            ids[5], masks[5] = -1, False
        instances.append(types.SimpleNamespace(gt_ids=ids, gt_classes=torch.arange(G) % 40, gt_masks=masks))
    batch = [{"image": frames, "instances": instances, "height": H, "width": W}]

    def step():
        m.zero_grad(set_to_none=True)
        torch.manual_seed(2)
        sum(m(batch).values()).backward()
    paths = {"kernel": step, "batched": with_env("0", step)}
    res = {k: [] for k in paths}
    for _ in range(a.repeats):
        for name, fn in paths.items():
            res[name].append(wall(fn, max(a.iters // 3, 3), warmup=2))
    line = {"step": "CTMinVIS R50 training step", "b": 1, "T": T, "G": G, "Q": 100, "frame": [H, W], "items": len(m.cl_plugin.last_items)}
    for name in paths:
        line[f"{name}_ms"] = round(float(np.median(res[name])), 2)
        line[f"{name}_spread_ms"] = round(max(res[name]) - min(res[name]), 2)
    line["batched_over_kernel"] = round(line["batched_ms"] / line["kernel_ms"], 3)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, default=None, metavar=("STEP", "B", "Q"), help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.child:
        if not torch.cuda.is_available():
            raise SystemExit("ctvis_train_time.py needs a GPU")
        kind, b, Q = a.child[0], int(a.child[1]), int(a.child[2])
        print("RESULT " + json.dumps(plugin_step(b, Q, a) if kind == "plugin" else full_step(a)), flush=True)
        return
    lines = []
    for kind, b, Q in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--repeats", str(a.repeats), "--child", kind, str(b), str(Q)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT[kind])
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {kind} b={b} Q={Q} ran into its time limit of {LIMIT[kind]} s: stopping")
        got = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"step {kind} b={b} Q={Q} failed (exit status {p.returncode}): stopping")
        print(got[0], flush=True)
        lines.append(got[0])
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
