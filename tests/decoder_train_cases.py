"""Golden g17 (tests/golden/gen_decoder_train_golden.py: the reference's masked-attention decoder in training mode) and the
training run both decoder-training test files replay on it."""
import ast
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRED_KEYS = ("pred_embds", "pred_embds_without_norm", "pred_reid_embed")


class G17:
    def __init__(self):
        load = lambda s: np.load(os.path.join(GOLDEN, f"g17_decoder_train{s}.npz"))
        self.z, self._state, self.preds, self._grads, self._grads_in = (load(s) for s in ("", "_state", "_preds", "_grads", "_grads_in"))
        self.meta = ast.literal_eval(str(self.z["meta"]))

    def t(self, key, z=None):
        return torch.from_numpy(np.asarray((self.z if z is None else z)[key]))

    def state(self):
        return {k: torch.from_numpy(self._state[k]) for k in self._state.files}

    def grads(self):
        return {k: torch.from_numpy(self._grads[k]) for k in self._grads.files}

    def grads_in(self):
        return {k: torch.from_numpy(self._grads_in[k]) for k in self._grads_in.files}

    def masks(self):
        return [self.t(f"mask/{i}") for i in range(self.meta["layers"])]

    def inputs(self, device="cpu", dtype=torch.float32):
        x = [self.t(f"in/x{i}").to(device, dtype) for i in range(3)]
        return x, self.t("in/mask_features").to(device, dtype)

    def cot(self, device="cpu", dtype=torch.float32):
        return {k: self.t(f"cot/{k}").to(device, dtype) for k in ("masks", "mask_weights", "logits", "embds", "reid")}


def build_decoder(g, device="cpu", dtype=torch.float32, cls="VideoMultiScaleMaskedTransformerDecoder_dvisPlus", state=None):
    from dvis_plus_amd import transformer_decoder as td
    m = g.meta
    kw = dict(num_classes=m["classes"], hidden_dim=m["hidden"], num_queries=m["Q"], nheads=m["heads"], dim_feedforward=m["ffn"],
              dec_layers=m["layers"], pre_norm=False, mask_dim=m["mask_dim"], enforce_input_project=False)
    if cls != "MultiScaleMaskedTransformerDecoder":
        kw["num_frames"] = m["num_frames"]
    if cls.endswith("dvisPlus"):
        kw.update(num_reid_head_layers=m["reid_layers"], reid_hidden_dim=m["hidden"])
    dec = getattr(td, cls)(m["hidden"], True, **kw)
    dec.load_state_dict(g.state() if state is None else state, strict=cls.endswith("dvisPlus"))
    return dec.to(device, dtype)


def predictions(out):
    """The L + 1 (pred_logits, pred_masks) pairs, the learnable queries' first."""
    return [(a["pred_logits"], a["pred_masks"]) for a in out["aux_outputs"]] + [(out["pred_logits"], out["pred_masks"])]


def loss_of(out, cot, C):
    """gen_decoder_train_golden.loss_of on the package's outputs: its pred_embds carries the re-id embedding in channels C .. 2C."""
    mean = lambda z, c: (z * c).sum() / z.numel()
    total = mean(out["pred_embds"][:, :C], cot["embds"]) + mean(out["pred_reid_embed"], cot["reid"])
    for i, (logits, masks) in enumerate(predictions(out)):
        total = total + mean(logits, cot["logits"][i]) + cot["mask_weights"][i] * mean(masks, cot["masks"])
    return total


def train_run(g, device="cpu", dtype=torch.float32, features_grad=True):
    """One training forward and backward of the g17 loss.  Returns (decoder, outputs, effective masks, {name: gradient}) with the
    gradients of every parameter, of the input maps ("x0" .. "x2") and, with features_grad, of "mask_features"."""
    dec = build_decoder(g, device, dtype).train()
    x, mf = g.inputs(device, dtype)
    x = [t.requires_grad_() for t in x]
    mf.requires_grad_(features_grad)
    dec.debug_masks = []
    out = dec(x, mf)
    masks, dec.debug_masks = dec.debug_masks, None
    loss_of(out, g.cot(device, dtype), g.meta["hidden"]).backward()
    grads = {n: p.grad for n, p in dec.named_parameters()}
    grads.update({f"x{i}": t.grad for i, t in enumerate(x)})
    if features_grad:
        grads["mask_features"] = mf.grad
    return dec, out, masks, grads


def check_predictions(g, out, tols):
    C = g.meta["hidden"]
    for tol in tols:
        for i, (logits, masks) in enumerate(predictions(out)):
            torch.testing.assert_close(logits.detach().cpu().float(), g.t(f"{i}/pred_logits", g.preds), **tol)
            torch.testing.assert_close(masks.detach().cpu().float(), g.t(f"{i}/pred_masks", g.preds), **tol)
        cpu = lambda k: out[k].detach().cpu().float()
        reid = g.t("pred_reid_embed", g.preds)
        torch.testing.assert_close(cpu("pred_reid_embed"), reid, **tol)
        for k in ("pred_embds", "pred_embds_without_norm"):           # the package concatenates the re-id embedding (its eval forward)
            torch.testing.assert_close(cpu(k)[:, :C], g.t(k, g.preds), **tol)
            torch.testing.assert_close(cpu(k)[:, C:], reid, **tol)


def golden_grads(g):
    want = g.grads()
    want.update(g.grads_in())
    return want
