"""Time the shifted-window attention kernel (csrc/window_attention.hip) against the reference's op sequence in torch on the same GPU,
and one Swin-L backbone forward with either.

    python tools/swin_time.py [--calls 20] [--repeats 5] [--out FILE]

One JSON line per measurement.  A window is --calls back-to-back calls between two hipEvents after 3 warm-up windows, `us` its time
per call; the two paths alternate --repeats times on the same device and the same tensors; the line holds the median of the repeats
and `spread` = (max - min).
  (a) window_attention   the Swin-L 720p stage shapes (token grids 180 x 320 / 90 x 160 / 45 x 80 / 23 x 40, C 192 .. 1536, head dim
      32, ws 12), shift 0 and 6, B = 1 and 5.  kernel: Fn.window_attention on the (B, H W, 3 C) qkv rows.  sequence: what swin.py does
      around its two Linear layers, as torch ops: F.pad, torch.roll, window partition of the (B, H, W, C) map (copies), then on the
      windows' qkv the permute, q scale, q k^T, the relative-position-bias gather and add, the mask add, softmax, P v, the transpose
      copy, then window reverse, the roll back and the crop.  (The mask matrix is built once outside: the reference builds it per stage.)
      `bound_us` = the larger of 16 C bytes / token at the HBM rate (8.0 TB/s) and 4 N C FLOP / token at the fp32 matrix peak (157.3
      TFLOP/s), `bound` says which; `share_of_bound` = bound_us / kernel_us.  `max_abs_diff` compares the two sides' output.
  (b) swinl_backbone_forward   D2SwinTransformer (EMBED_DIM 192, DEPTHS [2, 2, 18, 2], NUM_HEADS [6, 12, 24, 48], WINDOW_SIZE 12) on
      one 720 x 1280 frame: `kernel` as shipped, `formulation` with cpu_ops.window_attention's torch formulation on the GPU in the
      kernel's place.
No GPU -> the tool fails (it never times a CPU)."""
import argparse
import contextlib
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refiner_train_time import alternate                                                    # noqa: E402
from dvis_plus_amd import cpu_ops, d2, functions as Fn                                      # noqa: E402
from dvis_plus_amd.config import get_default_cfg                                            # noqa: E402

DEV = "cuda:0"
WS, D = 12, 32
STAGES = ((180, 320, 192), (90, 160, 384), (45, 80, 768), (23, 40, 1536))
HBM_BYTES_PER_S, F32_MATRIX_FLOPS = 8.0e12, 157.3e12


def partition(t, ws):
    B, Hp, Wp, C = t.shape
    return t.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws * ws, C)


def region_mask(Hp, Wp, ws, shift, device):
    img = torch.zeros((1, Hp, Wp, 1), device=device)
    cnt = 0
    for h in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for w in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, h, w, :] = cnt
            cnt += 1
    mw = partition(img, ws).view(-1, ws * ws)
    m = mw.unsqueeze(1) - mw.unsqueeze(2)
    return m.masked_fill(m != 0, -100.0).masked_fill(m == 0, 0.0)


class Sequence:
    """The reference's ops around qkv / proj for one block call.  `xn` is the normed (B, H, W, C) map the layout ops move; the
    attention itself runs on `qkv_win`, the projection of the partitioned windows (computed once, outside the timing: both sides
    leave the two Linear layers out)."""

    def __init__(self, xn, qkv_rows, qkv_bias, table, heads, ws, shift):
        self.xn, self.table, self.heads, self.ws, self.shift = xn, table, heads, ws, shift
        B, H, W, C = xn.shape
        self.pad = ((ws - W % ws) % ws, (ws - H % ws) % ws)
        Hp, Wp = H + self.pad[1], W + self.pad[0]
        q = qkv_bias.expand(B, Hp, Wp, 3 * C).clone()
        q[:, :H, :W] = qkv_rows.view(B, H, W, 3 * C)
        if shift:
            q = torch.roll(q, shifts=(-shift, -shift), dims=(1, 2))
        self.qkv_win = partition(q, ws)
        self.mask = region_mask(Hp, Wp, ws, shift, xn.device) if shift else None
        cy, cx = torch.meshgrid(torch.arange(ws, device=xn.device), torch.arange(ws, device=xn.device), indexing="ij")
        cy, cx = cy.flatten(), cx.flatten()
        self.index = ((cy[:, None] - cy[None, :] + ws - 1) * (2 * ws - 1) + (cx[:, None] - cx[None, :] + ws - 1)).view(-1)

    def __call__(self):
        ws, shift, heads = self.ws, self.shift, self.heads
        B, H, W, C = self.xn.shape
        N = ws * ws
        x = F.pad(self.xn, (0, 0, 0, self.pad[0], 0, self.pad[1]))
        Hp, Wp = x.shape[1:3]
        if shift:
            x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        partition(x, ws)                                                    # (its projection is self.qkv_win)
        B_ = self.qkv_win.shape[0]
        q, k, v = self.qkv_win.reshape(B_, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
        attn = (q * (C // heads) ** -0.5) @ k.transpose(-2, -1)
        attn = attn + self.table[self.index].view(N, N, -1).permute(2, 0, 1).contiguous().unsqueeze(0)
        if self.mask is not None:
            nW = self.mask.shape[0]
            attn = (attn.view(B_ // nW, nW, heads, N, N) + self.mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
        o = (torch.softmax(attn, dim=-1) @ v).transpose(1, 2).reshape(B_, N, C)
        o = o.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).contiguous().view(B, Hp, Wp, C)
        if shift:
            o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
        if self.pad[0] or self.pad[1]:
            o = o[:, :H, :W].contiguous()
        return o.view(B, H * W, C)


@contextlib.contextmanager
def torch_window_attention():
    """functions.window_attention = cpu_ops' torch formulation, for GPU tensors too (this tool's baseline only)."""
    kernel = Fn.window_attention
    Fn.window_attention = cpu_ops.window_attention
    try:
        yield
    finally:
        Fn.window_attention = kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swin_time.py needs a GPU")
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)
    gen = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        for H, W, C in STAGES:
            heads = C // D
            for B in (1, 5):
                xn = torch.randn(B, H, W, C, generator=gen, device=DEV)
                qkv = torch.randn(B, H * W, 3 * C, generator=gen, device=DEV)
                bias = 0.5 * torch.randn(3 * C, generator=gen, device=DEV)
                table = torch.randn((2 * WS - 1) ** 2, heads, generator=gen, device=DEV)
                for shift in (0, WS // 2):
                    seq = Sequence(xn, qkv, bias, table, heads, WS, shift)
                    kernel = lambda: Fn.window_attention(qkv, bias, table, B, H, W, heads, WS, shift)
                    err = float((kernel() - seq()).abs().max())
                    line = {"step": "window_attention", "B": B, "H": H, "W": W, "C": C, "heads": heads, "ws": WS, "shift": shift}
                    line.update(alternate((("kernel", kernel), ("sequence", seq)), a.calls, a.repeats))
                    tokens = B * H * W
                    t_mem, t_flop = tokens * 16 * C / HBM_BYTES_PER_S * 1e6, tokens * 4 * WS * WS * C / F32_MATRIX_FLOPS * 1e6
                    line["bound_us"], line["bound"] = round(max(t_mem, t_flop), 1), "fp32 matrix peak" if t_flop >= t_mem else "HBM"
                    line["share_of_bound"] = round(max(t_mem, t_flop) / line["kernel_us"], 3)
                    line["sequence_over_kernel"] = round(line["sequence_us"] / line["kernel_us"], 2)
                    line["max_abs_diff"] = err
                    emit(line)
                    del seq
                del xn, qkv
                torch.cuda.empty_cache()

        cfg = get_default_cfg()
        cfg.MODEL.BACKBONE.NAME = "D2SwinTransformer"
        cfg.MODEL.SWIN.merge({"EMBED_DIM": 192, "DEPTHS": [2, 2, 18, 2], "NUM_HEADS": [6, 12, 24, 48], "WINDOW_SIZE": 12,
                              "PRETRAIN_IMG_SIZE": 384})
        torch.manual_seed(0)
        bb = d2.build_backbone(cfg, None).to(DEV).eval()
        for m in bb.modules():
            if hasattr(m, "relative_position_bias_table"):
                m.relative_position_bias_table.normal_(0, 0.5)
                m.qkv.bias.normal_(0, 0.2)
        image = torch.randn(1, 3, 720, 1280, generator=gen, device=DEV)

        def forward():
            return bb(image)

        def forward_formulation():
            with torch_window_attention():
                return bb(image)
        want, got = forward_formulation(), forward()
        err = max(float((got[k] - want[k]).abs().max()) for k in got)
        line = {"step": "swinl_backbone_forward", "frames": 1, "size": [720, 1280], "depths": [2, 2, 18, 2], "ws": WS}
        line.update(alternate((("kernel", forward), ("formulation", forward_formulation)), max(1, a.calls // 4), a.repeats))
        line["formulation_over_kernel"] = round(line["formulation_us"] / line["kernel_us"], 3)
        line["max_abs_diff"] = err
        emit(line)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
