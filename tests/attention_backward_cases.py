"""The yardstick of tests/test_attention_backward_gpu.py and tests/test_masked_attention_backward_gpu.py: random inputs, the CPU
gradients they are measured against, and the check itself.

The reference is fp64 autograd of the ``cpu_ops.attention`` composition on the CPU (with the mask, where there is one).  The bound of
each of dq, dk, dv is measured, not chosen: 4 x the error of an fp32 CPU run against that fp64 run on the same inputs (4 = the
project's factor for a different summation order, tests/test_mask_gemm_backward_gpu.py).  The kernels' exponential is the hardware's
base-2 instruction where the CPU's is expf, so the fp32 CPU figure is the worse of two formulations per tensor: torch's softmax, and
the same composition with torch.exp2 on scores scaled by scale * log2(e).  It is never a kernel's own output.  Every compared tensor
has at least 64 elements (test_tracker_train_gpu.cpu_baselines says why)."""
import math

import torch


def draw(Lq, Lk, B, heads, d, seed, masked=True, open_fraction=0.25):
    """(q, k, v, grad_out, mask, allowed_count) from one seeded generator, drawn in that order; masked=False draws no mask (both
    None) and leaves the first four as they are with one."""
    gen = torch.Generator().manual_seed(seed)
    C = heads * d
    q, k, v, go = (torch.randn(L, B, C, generator=gen) for L in (Lq, Lk, Lk, Lq))
    mask = allowed = None
    if masked:
        mask = (torch.rand(B, Lq, Lk, generator=gen) >= open_fraction).to(torch.uint8)
        allowed = (mask == 0).sum(-1).to(torch.int32)
    return q, k, v, go, mask, allowed


def cpu_grads(q, k, v, go, heads, dtype, mask=None, allowed=None, base2=False):
    """(dq, dk, dv) by torch autograd of the cpu_ops.attention composition in `dtype`; base2: the softmax as exp2 on scores scaled
    by scale * log2(e), normalised by their sum (what the kernels compute)."""
    from dvis_plus_amd import cpu_ops
    q, k, v = (t.to(dtype).clone().requires_grad_() for t in (q, k, v))
    if not base2:
        out = cpu_ops.attention(q, k, v, heads, mask, allowed)
    else:
        Lq, B, C = q.shape
        Lk, d = k.shape[0], C // heads
        split = lambda t, n: t.reshape(n, B, heads, d).permute(1, 2, 0, 3)
        s = (split(q, Lq) @ split(k, Lk).transpose(-1, -2)) * ((1.0 / d ** 0.5) * math.log2(math.e))
        if mask is not None:
            s = s.masked_fill((mask.bool() & (allowed > 0)[..., None])[:, None], float("-inf"))
        e = torch.exp2(s - s.amax(-1, keepdim=True))
        out = ((e / e.sum(-1, keepdim=True)) @ split(v, Lk)).permute(2, 0, 1, 3).reshape(Lq, B, C)
    return torch.autograd.grad(out, (q, k, v), go.to(dtype))


def cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


def check_against_fp64(backward, q, k, v, go, heads, mask=None, allowed=None, label="", zero_error_takes_largest=True):
    """``backward(q, k, v, grad_out, heads[, mask, allowed])`` on the GPU copies of the inputs: every tensor within 4 x the worse fp32
    CPU formulation's error against fp64 autograd.  zero_error_takes_largest: a tensor whose fp32 CPU error is 0 (its exact gradient is
    0) takes the largest fp32 CPU error of the three as its baseline (the per-parameter check of tests/test_refiner_train_gpu.py sets
    the precedent); without it such a tensor must be exact.  Returns (the GPU gradients, the fp64 reference)."""
    ref = cpu_grads(q, k, v, go, heads, torch.float64, mask, allowed)
    a = cpu_grads(q, k, v, go, heads, torch.float32, mask, allowed)
    b = cpu_grads(q, k, v, go, heads, torch.float32, mask, allowed, base2=True)
    base = [max((x.double() - r).abs().max().item(), (y.double() - r).abs().max().item()) for x, y, r in zip(a, b, ref)]
    if zero_error_takes_largest:
        base = [e if e > 0 else max(base) for e in base]
    got = backward(*cuda(q, k, v, go), heads, *(cuda(mask, allowed) if mask is not None else ()))
    errs = []
    for name, x, r, e in zip(("dq", "dk", "dv"), got, ref, base):
        assert x.shape == r.shape and x.dtype == torch.float32 and x.is_contiguous() and r.numel() >= 64
        err = (x.cpu().double() - r).abs().max().item()
        errs.append(err)
        print(f"{label} {name}: err {err:.3e} fp32 CPU err {e:.3e} ratio {err / e if e else float(err > 0):.2f}")
    for name, err, e in zip(("dq", "dk", "dv"), errs, base):
        assert err <= 4 * e, f"{label} {name}: err {err:.3e} > 4 x {e:.3e}"          # (NaN fails)
    return got, ref
