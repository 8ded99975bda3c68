"""Op front-ends over the C ABI: the Python surface the reference's callers bind to.

``ms_deform_attn_forward`` / ``ms_deform_attn_backward`` have the signature of the reference's
pybind exports (ops/src/vision.cpp:18-21, ops/src/ms_deform_attn.h:25-66) and ``MSDeformAttnFunction``
that of ops/functions/ms_deform_attn_func.py:32-49, so ``MSDeformAttn`` / ViT-Adapter call sites work
unchanged.  Differences, all deliberate:
  * any batch size (the ``N % im2col_step`` assertion of ms_deform_attn_cuda.cu:55-57 is not needed;
    ``im2col_step`` is accepted and ignored),
  * fp16 / bf16 tensors are accepted in forward (fp32 accumulation) besides float / double,
  * failures raise ``RuntimeError`` — there is no torch/CPU fallback to hide them.
"""
import collections
import ctypes
import math
import os
import threading

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import cpu_ops, derived, native
from .cpu_ops import ms_deform_attn_core_pytorch    # noqa: F401  (the reference's name for the CPU-tensor formulation, ms_deform_attn_func.py:52)


def _torch_path(op, x, why):
    """Called where a fused glue op is about to take its torch formulation instead of the HIP kernel.  That is the right
    thing for CPU tensors (host-logic tests) and under autograd (the kernels are inference-only), and otherwise a shape /
    layout the kernel does not serve.  The latter RAISES (the default) instead of silently running torch ops on the GPU —
    the invisible dual path the reference has in ops/modules/ms_deform_attn.py:116-121.  DVIS_STRICT=0 is the explicit
    opt-out (odd research shapes: the torch formulation then runs, on the GPU)."""
    if os.environ.get("DVIS_STRICT", "1") != "0" and x.is_cuda and not torch.is_grad_enabled():
        raise RuntimeError(f"DVIS_STRICT: {op} would run its torch formulation on a GPU tensor ({why}; shape "
                           f"{tuple(x.shape)}, dtype {x.dtype}, contiguous {x.is_contiguous()})")


class no_autocast:
    """``with no_autocast(): ...`` — torch.autocast switched off (CUDA and CPU) for the enclosed calls: the fp32 island around the
    hand-written fp32 / split-f16 path.  The reference's launcher evaluates under ``with autocast():`` (train_net_video.py:259)
    and only its pixel decoder opts out (msdeformattn.py:314,320); here the WHOLE model does: under the launcher's context the
    results are the ones of the plain call, bit for bit (fp32 storage, within BASELINE's 1e-3 of the fp32 CPU reference — the
    reference's own GPU run is the half-precision one and is further from it)."""

    def __enter__(self):
        import contextlib
        self._stack = contextlib.ExitStack()
        self._stack.enter_context(torch.autocast(device_type="cuda", enabled=False))
        self._stack.enter_context(torch.autocast(device_type="cpu", enabled=False))
        return self

    def __exit__(self, *exc):
        return self._stack.__exit__(*exc)


def fp32_island(fn):
    """Decorator form of ``no_autocast`` for a module's ``forward`` (not for generators: a context must not stay entered
    across a ``yield`` — the consumer's code would run with autocast off)."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        if not (torch.is_autocast_enabled() or torch.is_autocast_enabled("cpu")):
            return fn(*args, **kwargs)
        with no_autocast():
            return fn(*args, **kwargs)
    return wrapper


def f32(t):
    """A half / double tensor handed over by an autocast region outside the island -> float32 (None and fp32 tensors pass)."""
    return t if t is None or not torch.is_tensor(t) or not t.is_floating_point() or t.dtype == torch.float32 else t.float()


def _check_msda_inputs(value, spatial_shapes, level_start_index, sampling_loc, attn_weight):
    for name, t in (("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
                    ("sampling_loc", sampling_loc), ("attn_weight", attn_weight)):
        if not t.is_contiguous():
            raise RuntimeError(f"{name} tensor has to be contiguous")
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a GPU tensor (no CPU implementation; got {t.device})")
    if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
        raise RuntimeError("spatial_shapes / level_start_index must be int64")
    if value.dim() != 4 or sampling_loc.dim() != 6 or attn_weight.dim() != 5:
        raise RuntimeError("expected value (N,S,M,D), sampling_loc (N,Lq,M,L,P,2), attn_weight (N,Lq,M,L,P)")
    if not (value.dtype == sampling_loc.dtype == attn_weight.dtype):
        raise RuntimeError("value, sampling_loc and attn_weight must share one dtype")
    N, S, M, D = value.shape
    N2, Lq, M2, L, P, two = sampling_loc.shape
    if (N2, M2, two) != (N, M, 2) or tuple(attn_weight.shape) != (N, Lq, M, L, P) or spatial_shapes.shape != (L, 2) \
            or level_start_index.shape != (L,):
        raise RuntimeError("inconsistent shapes between value / sampling_loc / attn_weight / spatial_shapes")
    return N, S, M, D, L, Lq, P


def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step=128):
    """-> (N, Lq, M*D).  Drop-in for ``MultiScaleDeformableAttention.ms_deform_attn_forward``."""
    N, S, M, D, L, Lq, P = _check_msda_inputs(value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
    out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
    with torch.cuda.device(value.device):
        rc = native.lib().dvis_msda_forward(
            native.dtype_code(value), native.dev_ptr(value, "value"), native.dev_ptr(spatial_shapes, "spatial_shapes"),
            native.dev_ptr(level_start_index, "level_start_index"), native.dev_ptr(sampling_loc, "sampling_loc"),
            native.dev_ptr(attn_weight, "attn_weight"), N, S, M, D, L, Lq, P, native.dev_ptr(out, "out"),
            native.stream_ptr(value.device))
    native.check(rc, "dvis_msda_forward")
    return out


# Reproducible MSDeformAttn backward (fp32): 1 = always, 0 = never, default = when torch.use_deterministic_algorithms(True) is set.
MSDA_BWD_DETERMINISTIC = os.environ.get("DVIS_MSDA_BWD_DETERMINISTIC")


def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output,
                            im2col_step=128, deterministic=None):
    """-> [grad_value, grad_sampling_loc, grad_attn_weight] (ops/src/ms_deform_attn.h:47-66).
    deterministic (fp32): grad_value through 64-bit fixed-point integer atomics (dvis_msda_backward_det) — the same bits every run;
    default: DVIS_MSDA_BWD_DETERMINISTIC, else torch.are_deterministic_algorithms_enabled()."""
    N, S, M, D, L, Lq, P = _check_msda_inputs(value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
    if not grad_output.is_cuda:
        raise RuntimeError("grad_output must be a GPU tensor")
    grad_output = grad_output.contiguous()
    if grad_output.dtype != value.dtype or grad_output.numel() != N * Lq * M * D:
        raise RuntimeError("grad_output must be (N, Lq, M*D) with value's dtype")
    if deterministic is None:
        deterministic = (MSDA_BWD_DETERMINISTIC == "1") if MSDA_BWD_DETERMINISTIC in ("0", "1") \
            else torch.are_deterministic_algorithms_enabled()
    grad_loc = torch.empty_like(sampling_loc)
    grad_w = torch.empty_like(attn_weight)
    if deterministic and value.dtype == torch.float32:
        grad_value = torch.empty_like(value)
        nbytes = native.lib().dvis_msda_backward_det_ws_bytes(N, S, M, D)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=value.device)
        with torch.cuda.device(value.device):
            rc = native.lib().dvis_msda_backward_det(
                native.dev_ptr(value, "value"), native.dev_ptr(spatial_shapes, "spatial_shapes"),
                native.dev_ptr(level_start_index, "level_start_index"), native.dev_ptr(sampling_loc, "sampling_loc"),
                native.dev_ptr(attn_weight, "attn_weight"), native.dev_ptr(grad_output, "grad_output"),
                N, S, M, D, L, Lq, P, native.dev_ptr(grad_value, "grad_value"), native.dev_ptr(grad_loc, "grad_loc"),
                native.dev_ptr(grad_w, "grad_w"), ctypes.c_void_p(ws.data_ptr()), native.stream_ptr(value.device))
        native.check(rc, "dvis_msda_backward_det")
        return [grad_value, grad_loc, grad_w]
    grad_value = torch.zeros_like(value)
    with torch.cuda.device(value.device):
        rc = native.lib().dvis_msda_backward(
            native.dtype_code(value), native.dev_ptr(value, "value"), native.dev_ptr(spatial_shapes, "spatial_shapes"),
            native.dev_ptr(level_start_index, "level_start_index"), native.dev_ptr(sampling_loc, "sampling_loc"),
            native.dev_ptr(attn_weight, "attn_weight"), native.dev_ptr(grad_output, "grad_output"),
            N, S, M, D, L, Lq, P, native.dev_ptr(grad_value, "grad_value"), native.dev_ptr(grad_loc, "grad_loc"),
            native.dev_ptr(grad_w, "grad_w"), native.stream_ptr(value.device))
    native.check(rc, "dvis_msda_backward")
    return [grad_value, grad_loc, grad_w]


class MSDeformAttnFunction(Function):
    """Same contract as the reference's autograd wrapper (ops/functions/ms_deform_attn_func.py:32-49)."""

    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights,
                im2col_step):
        ctx.im2col_step = im2col_step
        output = ms_deform_attn_forward(value, value_spatial_shapes, value_level_start_index, sampling_locations,
                                        attention_weights, im2col_step)
        ctx.save_for_backward(value, value_spatial_shapes, value_level_start_index, sampling_locations,
                              attention_weights)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, shapes, level_start, loc, w = ctx.saved_tensors
        grad_value, grad_loc, grad_w = ms_deform_attn_backward(value, shapes, level_start, loc, w, grad_output,
                                                               ctx.im2col_step)
        return grad_value, None, None, grad_loc, grad_w, None


def msda_fused_forward(value, spatial_shapes, level_start_index, reference_points, offsets, logits, n_levels,
                       n_points, shapes_host=None):
    """Inference fast path of ``MSDeformAttn.forward`` (ops/modules/ms_deform_attn.py:101-117): fp32, or fp16 / bf16
    storage with fp32 arithmetic (value, offsets, logits and the output in ONE dtype — the module under autocast).

    value (N,S,M,D); reference_points (1|N, Lq, L, 2); ``offsets`` / ``logits`` are 2-D row views
    (N*Lq, >= M*L*P*2) / (N*Lq, >= M*L*P) of the raw linear outputs (row stride may exceed the width, e.g.
    both sliced out of one fused projection).  softmax + location arithmetic happen inside the kernel.
    shapes_host: optional [(H, W), ...] python copy of spatial_shapes (enables 8x8 query tiling for self-attention).
    """
    N, S, M, D = value.shape
    L, P = n_levels, n_points
    nref, Lq = reference_points.shape[0], reference_points.shape[1]
    for name, t in (("value", value), ("reference_points", reference_points)):
        native.dev_ptr(t, name)
    for name, t in (("offsets", offsets), ("logits", logits)):
        if not t.is_cuda or t.dtype != value.dtype or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != N * Lq:
            raise RuntimeError(f"{name} must be a GPU (N*Lq, width) row view of value's dtype with unit inner stride")
    if value.dtype not in (torch.float32, torch.float16, torch.bfloat16) or reference_points.dtype != torch.float32:
        raise RuntimeError("msda_fused_forward: value / offsets / logits fp32, fp16 or bf16 (one dtype); reference points fp32")
    if offsets.shape[1] < M * L * P * 2 or logits.shape[1] < M * L * P or reference_points.shape[2:] != (L, 2):
        raise RuntimeError("msda_fused_forward: inconsistent shapes")
    out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
    hs = None
    if shapes_host is not None:
        hs = (ctypes.c_int64 * (2 * L))(*[int(v) for hw in shapes_host for v in hw])
    with torch.cuda.device(value.device):
        rc = native.lib().dvis_msda_fused_forward(
            native.dtype_code(value), native.dev_ptr(value, "value"), native.dev_ptr(spatial_shapes, "spatial_shapes"),
            native.dev_ptr(level_start_index, "level_start_index"), native.dev_ptr(reference_points, "ref"), nref,
            ctypes.c_void_p(offsets.data_ptr()), offsets.stride(0), ctypes.c_void_p(logits.data_ptr()), logits.stride(0),
            N, S, M, D, L, Lq, P, native.dev_ptr(out, "out"), hs, native.stream_ptr(value.device))
    native.check(rc, "dvis_msda_fused_forward")
    return out


def msda_fused_backward_ok(x, head_dim, n_levels, n_points):
    """The domain of ``msda_fused_backward`` (the fused forward's fp32 domain) for projections of the tensor `x`: the caller's
    dispatch test — outside it the unfused ``MSDeformAttnFunction`` is the op under autograd."""
    return (x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled() and head_dim in (32, 64)
            and (n_levels, n_points) in ((1, 4), (3, 4), (4, 4)))


def msda_fused_backward(value, spatial_shapes, level_start_index, reference_points, offsets, logits, grad_out, n_levels,
                        n_points, deterministic=None):
    """Backward of ``msda_fused_forward`` in its fp32 domain (D in {32, 64}, (L, P) in {(1,4), (3,4), (4,4)})
    -> (grad_value (N,S,M,D), grad_offsets (N*Lq, M*L*P*2), grad_logits (N*Lq, M*L*P)).  The inputs are
    the forward's own — the RAW row views — and the kernel recomputes softmax and locations: no (N, Lq, M, L, P, 3) tensor is
    read or written.  The reference points get no gradient.  deterministic: as ``ms_deform_attn_backward`` (grad_offsets /
    grad_logits are the same bits either way)."""
    if value.dim() != 4:
        raise RuntimeError("msda_fused_backward: value must be (N, S, M, D)")
    N, S, M, D = value.shape
    L, P = int(n_levels), int(n_points)
    if reference_points.requires_grad:
        raise RuntimeError("msda_fused_backward: the reference points get no gradient (requires_grad is set)")
    if reference_points.dim() != 4 or reference_points.shape[2:] != (L, 2) or reference_points.shape[0] not in (1, N):
        raise RuntimeError("msda_fused_backward: reference_points must be (1|N, Lq, L, 2)")
    nref, Lq = reference_points.shape[0], reference_points.shape[1]
    for name, t in (("value", value), ("reference_points", reference_points), ("spatial_shapes", spatial_shapes),
                    ("level_start_index", level_start_index)):
        native.dev_ptr(t, name)
    if value.dtype != torch.float32 or reference_points.dtype != torch.float32:
        raise RuntimeError("msda_fused_backward: fp32 only")
    if D not in (32, 64) or (L, P) not in ((1, 4), (3, 4), (4, 4)):
        raise RuntimeError(f"msda_fused_backward: unsupported (D={D}, L={L}, P={P}); supported D in {{32,64}}, "
                           "(L,P) in {(1,4),(3,4),(4,4)}")
    for name, t, width in (("offsets", offsets, M * L * P * 2), ("logits", logits, M * L * P)):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != N * Lq \
                or t.shape[1] < width:
            raise RuntimeError(f"{name} must be a float32 GPU (N*Lq, >= {width}) row view with unit inner stride")
        if t.data_ptr() % 16 or (t.shape[0] > 1 and t.stride(0) % 4):
            raise RuntimeError(f"msda_fused_backward: {name} rows must be 16-byte aligned (row stride a multiple of 4 floats)")
    if not grad_out.is_cuda or grad_out.dtype != torch.float32 or grad_out.numel() != N * Lq * M * D:
        raise RuntimeError("grad_out must be a float32 GPU (N, Lq, M*D) tensor")
    grad_out = grad_out.contiguous()
    if deterministic is None:
        deterministic = (MSDA_BWD_DETERMINISTIC == "1") if MSDA_BWD_DETERMINISTIC in ("0", "1") \
            else torch.are_deterministic_algorithms_enabled()
    grad_value = torch.empty_like(value, memory_format=torch.contiguous_format)
    grad_off = torch.empty((N * Lq, M * L * P * 2), dtype=torch.float32, device=value.device)
    grad_logit = torch.empty((N * Lq, M * L * P), dtype=torch.float32, device=value.device)
    ws = None
    if deterministic:
        nbytes = native.lib().dvis_msda_fused_backward_ws_bytes(N, S, M, D)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=value.device)
    with torch.cuda.device(value.device):
        rc = native.lib().dvis_msda_fused_backward(
            native.dev_ptr(value, "value"), native.dev_ptr(spatial_shapes, "spatial_shapes"),
            native.dev_ptr(level_start_index, "level_start_index"), native.dev_ptr(reference_points, "ref"), nref,
            ctypes.c_void_p(offsets.data_ptr()), offsets.stride(0), ctypes.c_void_p(logits.data_ptr()), logits.stride(0),
            native.dev_ptr(grad_out, "grad_out"), N, S, M, D, L, Lq, P, native.dev_ptr(grad_value, "grad_value"),
            native.dev_ptr(grad_off, "grad_offsets"), native.dev_ptr(grad_logit, "grad_logits"),
            None if ws is None else ctypes.c_void_p(ws.data_ptr()), native.stream_ptr(value.device))
    native.check(rc, "dvis_msda_fused_backward")
    return grad_value, grad_off, grad_logit


class MSDAFusedFunction(Function):
    """``msda_fused_forward`` under autograd: saves value, the two raw row views and the reference points — no locations, no
    weights, no output — and ``msda_fused_backward`` recomputes the rest."""

    @staticmethod
    def forward(ctx, value, offsets, logits, spatial_shapes, level_start_index, reference_points, n_levels, n_points,
                shapes_host):
        ctx.n_levels, ctx.n_points = n_levels, n_points
        out = msda_fused_forward(value, spatial_shapes, level_start_index, reference_points, offsets, logits, n_levels,
                                 n_points, shapes_host)
        ctx.save_for_backward(value, offsets, logits, spatial_shapes, level_start_index, reference_points)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        value, offsets, logits, shapes, level_start, ref = ctx.saved_tensors
        gv, go, gl = msda_fused_backward(value, shapes, level_start, ref, offsets, logits, grad_out, ctx.n_levels, ctx.n_points)
        M, LP = value.shape[2], ctx.n_levels * ctx.n_points
        # the row views may be wider than a head run (slices of one projection): the gradient has the view's shape
        if offsets.shape[1] != M * LP * 2:
            go = torch.nn.functional.pad(go, (0, offsets.shape[1] - M * LP * 2))
        if logits.shape[1] != M * LP:
            gl = torch.nn.functional.pad(gl, (0, logits.shape[1] - M * LP))
        return gv, go, gl, None, None, None, None, None, None


def _msda_fused_torch(value, spatial_shapes, reference_points, offsets, logits, L, P):
    """The torch formulation of the fused op (ops/modules/ms_deform_attn.py:101-117) for CPU tensors."""
    N, S, M, D = value.shape
    Lq = reference_points.shape[1]
    off = offsets[:, :M * L * P * 2].reshape(N, Lq, M, L, P, 2)
    w = torch.softmax(logits[:, :M * L * P].reshape(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
    norm = torch.stack([spatial_shapes[..., 1], spatial_shapes[..., 0]], -1).to(value.dtype)
    loc = reference_points[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    return cpu_ops.ms_deform_attn_core_pytorch(value, spatial_shapes, loc.expand(N, -1, -1, -1, -1, -1), w)


def msda_fused(value, spatial_shapes, level_start_index, reference_points, offsets, logits, n_levels, n_points,
               shapes_host=None):
    """``msda_fused_forward`` that also trains: without a requires-grad input it IS that call (the same bits); with one it is
    ``MSDAFusedFunction`` (forward = that same call, backward = ``msda_fused_backward``).  CPU tensors take the torch
    formulation and torch's autograd.  A ``reference_points`` that requires grad raises: the kernel has no gradient for it."""
    if reference_points.requires_grad:
        raise RuntimeError("msda_fused: reference_points must not require grad (the fused backward has no gradient for them)")
    if _on_cpu(value, offsets, logits, reference_points):
        return _msda_fused_torch(value, spatial_shapes, reference_points, offsets, logits, n_levels, n_points)
    if not (torch.is_grad_enabled() and (value.requires_grad or offsets.requires_grad or logits.requires_grad)):
        return msda_fused_forward(value, spatial_shapes, level_start_index, reference_points, offsets, logits, n_levels,
                                  n_points, shapes_host)
    if not (msda_fused_backward_ok(value, value.shape[3], n_levels, n_points) and offsets.dtype == logits.dtype == torch.float32):
        raise RuntimeError("msda_fused: under autograd only the fp32 domain of msda_fused_backward is served (D in {32,64}, "
                           "(L,P) in {(1,4),(3,4),(4,4)}); use MSDeformAttnFunction")
    return MSDAFusedFunction.apply(value, offsets, logits, spatial_shapes, level_start_index, reference_points,
                                   int(n_levels), int(n_points), shapes_host)


def _on_cpu(*tensors):
    """Every tensor lives on the CPU: the call takes the torch formulation of cpu_ops.py (BASELINE config #1, "PyTorch CPU
    MSDeformAttn fallback (plumbing, no GPU)").  Decided by DEVICE alone: a GPU tensor never ends up there — the HIP kernel runs
    or the call raises."""
    return all(t.device.type == "cpu" for t in tensors)


def _f32_gpu(t, name):
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
    return native.dev_ptr(t, name)


def _mask_logits_kernel(mask_embed, mask_features):
    B, Q, C = mask_embed.shape
    H, W = mask_features.shape[-2:]
    pe, pf = _f32_gpu(mask_embed, "mask_embed"), _f32_gpu(mask_features, "mask_features")
    out = torch.empty((B, Q, H, W), dtype=torch.float32, device=mask_embed.device)
    with torch.cuda.device(mask_embed.device):
        rc = native.lib().dvis_mask_logits(pe, pf, B, Q, C, H * W, native.dev_ptr(out, "out"),
                                           native.stream_ptr(mask_embed.device))
    native.check(rc, "dvis_mask_logits")
    return out


def mask_logits_backward(grad_logits, mask_features):
    """Backward of ``mask_logits`` with respect to ``mask_embed`` (csrc/mask_gemm_backward.hip): grad_logits (B, R, H, W) and
    mask_features (B, C, H, W), contiguous float32 GPU tensors -> (grad_embed (B, R, C) = einsum("brp,bcp->brc"), row_sum (B, R) =
    grad_logits summed over the pixels).  Exact fp32, and the same bits on every call: the pixels are cut into slabs by their
    number alone and the slabs' partial results are added in order — no atomics."""
    B, R = grad_logits.shape[:2]
    Bf, C, H, W = mask_features.shape
    if Bf != B or grad_logits.numel() != B * R * H * W:
        raise RuntimeError("mask_logits_backward: grad_logits (B,R,H,W) and mask_features (B,C,H,W) disagree")
    pg, pf = _f32_gpu(grad_logits, "grad_logits"), _f32_gpu(mask_features, "mask_features")
    dev = grad_logits.device
    grad_embed = torch.empty((B, R, C), dtype=torch.float32, device=dev)
    row_sum = torch.empty((B, R), dtype=torch.float32, device=dev)
    lib = native.lib()
    nbytes = lib.dvis_mask_logits_backward_ws_bytes(B, R, C, H * W)
    # per call (46 MB at the training shape): torch's caching allocator hands the same block back step after step
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        rc = lib.dvis_mask_logits_backward(pg, pf, B, R, C, H * W, native.dev_ptr(grad_embed, "grad_embed"),
                                           native.dev_ptr(row_sum, "row_sum"),
                                           ctypes.c_void_p(ws.data_ptr()) if ws is not None else None, native.stream_ptr(dev))
    native.check(rc, "dvis_mask_logits_backward")
    return grad_embed, row_sum


def _mask_logits_grad_features(mask_embed, grad_logits):
    """einsum("bqc,bqhw->bchw"): the forward contraction with mask_embed transposed and the logit gradient as the map."""
    Q = mask_embed.shape[1]
    if Q > 256:
        raise RuntimeError(f"mask_logits: the gradient with respect to mask_features contracts over the {Q} rows of mask_embed on "
                           "the forward kernel, which serves at most 256; detach mask_features (a frozen segmenter's map needs no "
                           "gradient) or call it with fewer rows")
    return _mask_logits_kernel(mask_embed.transpose(1, 2).contiguous(), grad_logits)


class MaskLogitsFunction(Function):
    """``mask_logits`` under autograd: the forward kernel, csrc/mask_gemm_backward.hip for mask_embed, the forward kernel on
    transposed operands for mask_features."""

    @staticmethod
    def forward(ctx, mask_embed, mask_features):
        ctx.save_for_backward(mask_embed, mask_features)
        return _mask_logits_kernel(mask_embed, mask_features)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_logits):
        mask_embed, mask_features = ctx.saved_tensors
        grad_logits = grad_logits.contiguous()
        g_embed = g_feat = None
        if ctx.needs_input_grad[0]:
            g_embed, _ = mask_logits_backward(grad_logits, mask_features)
        if ctx.needs_input_grad[1]:
            g_feat = _mask_logits_grad_features(mask_embed, grad_logits)
        return g_embed, g_feat


def mask_logits(mask_embed, mask_features):
    """einsum("bqc,bchw->bqhw") of forward_prediction_heads
    (dvis_Plus/video_mask2former_transformer_decoder.py:363), exact-fp32 MFMA.  (B,Q,C) x (B,C,H,W) -> (B,Q,H,W).
    Differentiable: an input that requires grad gets its gradient from MaskLogitsFunction (CPU tensors: torch's own)."""
    B, Q, C = mask_embed.shape
    Bf, Cf, H, W = mask_features.shape
    if (Bf, Cf) != (B, C):
        raise RuntimeError("mask_logits: mask_embed (B,Q,C) and mask_features (B,C,H,W) disagree")
    if _on_cpu(mask_embed, mask_features):
        return cpu_ops.mask_logits(mask_embed, mask_features)
    if torch.is_grad_enabled() and (mask_embed.requires_grad or mask_features.requires_grad):
        _f32_gpu(mask_embed, "mask_embed"), _f32_gpu(mask_features, "mask_features")
        return MaskLogitsFunction.apply(mask_embed, mask_features)
    return _mask_logits_kernel(mask_embed, mask_features)


class ProjectedMaskLogitsFunction(Function):
    """``projected_mask_logits`` on the GPU: see there for the formulas."""

    @staticmethod
    def forward(ctx, mask_embed, feat, weight, bias):
        e2 = torch.matmul(mask_embed, weight).contiguous()                    # E' = mask_embed W   (B, R, C_in)
        logits = _mask_logits_kernel(e2, feat)
        if bias is not None:
            logits += torch.matmul(mask_embed, bias)[..., None, None]
        ctx.save_for_backward(mask_embed, feat, weight, bias)
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_logits):
        mask_embed, feat, weight, bias = ctx.saved_tensors
        if ctx.needs_input_grad[1]:
            raise RuntimeError("projected_mask_logits: no gradient for the feature map (the segmenter is frozen in the tracker's "
                               "training stage); detach it")
        g_e2, row_sum = mask_logits_backward(grad_logits.contiguous(), feat)   # dE' = g feat^T, sum_p g
        g_embed = g_w = g_b = None
        if ctx.needs_input_grad[0]:
            g_embed = torch.matmul(g_e2, weight.t())
            if bias is not None:
                g_embed = g_embed + row_sum[..., None] * bias
        if ctx.needs_input_grad[2]:
            g_w = torch.matmul(mask_embed.flatten(0, 1).t(), g_e2.flatten(0, 1))
        if bias is not None and ctx.needs_input_grad[3]:
            g_b = torch.matmul(mask_embed.flatten(0, 1).t(), row_sum.flatten())
        return g_embed, None, g_w, g_b


def projected_mask_logits(mask_embed, feat, weight, bias=None):
    """``mask_logits(mask_embed, conv1x1(feat, weight, bias))`` — the tracker's mask head on its own 1 x 1 projection of the
    segmenter's map (dvis_Plus/tracker.py:199, :379) — WITHOUT the projected map or its gradient ever existing:
        E' = mask_embed W                      logits = E' feat + (mask_embed b)[..., None]
        dE' = g feat^T  (csrc/mask_gemm_backward.hip, with row_sum = sum_p g)
        d mask_embed = dE' W^T + row_sum (x) b      dW = sum mask_embed^T dE'      db = sum mask_embed^T row_sum
    mask_embed (B, R, C_out), feat (B, C_in, H, W) [no gradient: the segmenter is frozen], weight (C_out, C_in[, 1, 1]), bias
    (C_out) -> (B, R, H, W).  Everything but the two contractions over the pixels is R x C sized arithmetic.  The summation order
    differs from project-then-contract by fp32 rounding only."""
    B, R, Co = mask_embed.shape
    weight = weight.reshape(weight.shape[0], -1)
    if weight.shape[0] != Co or feat.shape[:2] != (B, weight.shape[1]):
        raise RuntimeError("projected_mask_logits: mask_embed (B,R,Co), feat (B,Ci,H,W) and weight (Co,Ci) disagree")
    if _on_cpu(mask_embed, feat, weight):
        logits = cpu_ops.mask_logits(torch.matmul(mask_embed, weight), feat)
        return logits if bias is None else logits + torch.matmul(mask_embed, bias)[..., None, None]
    _f32_gpu(mask_embed, "mask_embed"), _f32_gpu(feat, "feat")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (mask_embed, feat, weight, bias)):
        return ProjectedMaskLogitsFunction.apply(mask_embed, feat, weight, bias)
    with torch.no_grad():
        return ProjectedMaskLogitsFunction.forward(_NoCtx(), mask_embed, feat, weight, bias)


class _NoCtx:
    def save_for_backward(self, *tensors):
        pass


def attn_mask(mask_embed, mask_features, target_size):
    """Attention mask of the next decoder layer in ONE launch: contraction + bilinear down-sizing + threshold
    (ibid. :363-371).  Returns (mask uint8 (B,Q,h*w) with 1 = blocked — a single copy, not repeated per head —,
    allowed_count int32 (B,Q)); a row with allowed_count == 0 must be treated as un-masked (:297), which
    ``attention`` does on the device."""
    B, Q, C = mask_embed.shape
    Bf, Cf, H, W = mask_features.shape
    h, w = int(target_size[0]), int(target_size[1])
    if (Bf, Cf) != (B, C):
        raise RuntimeError("attn_mask: mask_embed (B,Q,C) and mask_features (B,C,H,W) disagree")
    if _on_cpu(mask_embed, mask_features):
        return cpu_ops.attn_mask(mask_embed, mask_features, (h, w))
    pe, pf = _f32_gpu(mask_embed, "mask_embed"), _f32_gpu(mask_features, "mask_features")
    mask = torch.empty((B, Q, h * w), dtype=torch.uint8, device=mask_embed.device)
    allowed = torch.empty((B, Q), dtype=torch.int32, device=mask_embed.device)
    with torch.cuda.device(mask_embed.device):
        rc = native.lib().dvis_attn_mask(pe, pf, B, Q, C, H, W, h, w, native.dev_ptr(mask, "mask"),
                                         native.dev_ptr(allowed, "allowed"), native.stream_ptr(mask_embed.device))
    native.check(rc, "dvis_attn_mask")
    return mask, allowed


ATTN_MASK_PYRAMID = os.environ.get("DVIS_ATTN_MASK_PYRAMID", "1") != "0"


def center_pool3(mask_features):
    """The decoder's attention-mask pyramid, once per call of the decoder: (p8, p4, p2) — low resolution first, the decoder's
    level order — with p_s[n, c, i, j] = 0.25 * ((f_a + f_b) + (f_c + f_d)) over the four centre pixels of block (i, j) of s x s
    pixels: what F.interpolate(bilinear, align_corners=False) to 1/s samples, on the FEATURES (the contraction is linear).  None
    when the map is not served (H, W not multiples of 8, CPU tensors, autograd): the caller uses ``attn_mask``."""
    if not (ATTN_MASK_PYRAMID and mask_features.is_cuda and mask_features.dtype == torch.float32 and mask_features.dim() == 4
            and mask_features.is_contiguous() and not torch.is_grad_enabled()):
        return None
    N, C, H, W = mask_features.shape
    if H % 8 or W % 8 or mask_features.data_ptr() % 16:
        return None
    p2 = torch.empty((N, C, H // 2, W // 2), dtype=torch.float32, device=mask_features.device)
    p4 = torch.empty((N, C, H // 4, W // 4), dtype=torch.float32, device=mask_features.device)
    p8 = torch.empty((N, C, H // 8, W // 8), dtype=torch.float32, device=mask_features.device)
    if N:
        with torch.cuda.device(mask_features.device):
            native.check(native.lib().dvis_center_pool3(native.dev_ptr(mask_features, "mask_features"), N * C, H, W,
                                                        native.dev_ptr(p2, "p2"), native.dev_ptr(p4, "p4"), native.dev_ptr(p8, "p8"),
                                                        native.stream_ptr(mask_features.device)), "dvis_center_pool3")
    return p8, p4, p2


def attn_mask_pooled(mask_embed, pooled):
    """``attn_mask`` on a level's pooled map (center_pool3): (mask uint8 (B, Q, h*w), allowed_count int32 (B, Q))."""
    B, Q, C = mask_embed.shape
    Bf, Cf, h, w = pooled.shape
    if (Bf, Cf) != (B, C):
        raise RuntimeError("attn_mask_pooled: mask_embed (B,Q,C) and pooled (B,C,h,w) disagree")
    pe, pf = _f32_gpu(mask_embed, "mask_embed"), _f32_gpu(pooled, "pooled")
    mask = torch.empty((B, Q, h * w), dtype=torch.uint8, device=mask_embed.device)
    allowed = torch.empty((B, Q), dtype=torch.int32, device=mask_embed.device)
    with torch.cuda.device(mask_embed.device):
        native.check(native.lib().dvis_attn_mask_pooled(pe, pf, B, Q, C, h, w, native.dev_ptr(mask, "mask"),
                                                        native.dev_ptr(allowed, "allowed"), native.stream_ptr(mask_embed.device)),
                     "dvis_attn_mask_pooled")
    return mask, allowed


MaskGemmPass = collections.namedtuple("MaskGemmPass", "qbeg QT fullc vec gpf spf total_steps nwg")


def mask_gemm_plan(mode, B, Q, C, H, W, h=0, w=0, aligned=True, embed_aligned=True):
    """How csrc/mask_gemm.hip would run ``mask_logits`` (mode 0, map H x W), ``attn_mask`` (mode 1, H x W -> h x w) or
    ``attn_mask_pooled`` (mode 2, pooled map H x W; h, w unused), without launching it: one MaskGemmPass per pass over the queries —
    qbeg (its first query), QT (query tiles of the kernel instantiation: 2, 4 or 7), fullc (no per-channel selects and 16-byte
    reads of mask_embed: C % 32 == 0 and ``embed_aligned``), vec (16-byte map loads and packed stores: modes 0 and 2, H W % 4 == 0,
    ``aligned``, fullc), gpf / spf (wave groups and steps of 8 groups per frame), total_steps (B * spf) and nwg (the workgroups
    that share the steps out).  ``aligned``: the map and the output start on 16 bytes; ``embed_aligned``: so does mask_embed.  The
    answer comes from dvis_mask_gemm_plan, the function the launch itself consults; only shapes are read, so no GPU is needed."""
    cap = 8
    while True:
        buf = (ctypes.c_int32 * (1 + 8 * cap))()
        rc = native.lib().dvis_mask_gemm_plan(mode, B, Q, C, H, W, h, w, int(aligned), int(embed_aligned), buf, cap)
        native.check(rc, "dvis_mask_gemm_plan")
        if buf[0] <= cap:
            words = [buf[1 + 8 * i:9 + 8 * i] for i in range(buf[0])]
            return tuple(MaskGemmPass(p[0], p[1], bool(p[2]), bool(p[3]), *p[4:]) for p in words)
        cap = buf[0]


def _strides3(t, B, C, d):
    """(L, B, C) tensor -> {batch, head, row} strides in floats for the kernel's (B, heads, L, d) view."""
    return (ctypes.c_int64 * 3)(t.stride(1) if B > 1 else C, d, t.stride(0))


def attention(q, k, v, nheads, mask=None, allowed_count=None, out=None, short=False):
    """Multi-head softmax(q k^T / sqrt(d)) v on projected, sequence-first tensors (what
    nn.MultiheadAttention computes between its in- and out-projection).

    q (Lq, B, C), k / v (Lk, B, C) float32 GPU tensors whose last dim is contiguous — arbitrary row / batch
    strides, so slices of a fused in-projection work without copies; heads are the C = nheads * d split,
    d in {32, 64}.  mask: uint8 / bool (B, Lq, Lk), 1 = blocked, shared by all heads of a batch entry;
    allowed_count int32 (B, Lq) from ``attn_mask`` (rows with 0 ignore the mask).
    Returns (Lq, B, C) ready for the out-projection.
    short=True pins the short-key latency kernel (Lk <= 128) whatever the batch size: same bits per (batch, head) for a clip
    alone or stacked with others (the tracker's recurrence).
    Differentiable without a mask: an input that requires grad routes the call through AttentionFunction (same forward kernel,
    same bits; CPU tensors: torch's own autograd).
    """
    if _on_cpu(q, k, v):
        return cpu_ops.attention(q, k, v, nheads, mask, allowed_count, out)
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        if mask is not None:
            raise RuntimeError("attention: no gradient through a masked attention (csrc/attention_backward.hip serves mask=None); "
                               "detach q / k / v or call it without a mask")
        if out is not None:
            raise RuntimeError("attention: out= cannot be combined with an input that requires grad (the result must be a new "
                               "tensor of the autograd graph)")
        _attention_backward_check(q, k, v, None, nheads)
        return AttentionFunction.apply(q, k, v, nheads, None, None, short, False)
    return _attention_kernel(q, k, v, nheads, mask, allowed_count, out, short)


def _attention_kernel_arg(Lq, Lk, d, has_mask, short):
    """The `kernel` argument of dvis_attention_forward_k for a call: 1 = the pinned short-key kernel, 2 = split-f16, 0 = the library's
    own choice from the sizes."""
    if short:
        return 1
    if not has_mask and d == 64 and Lq >= 1024 and Lk >= 1024 and x3_on():
        # long self-attention at head dim 64 (the DINOv2 / ViT-Adapter blocks: 3681 tokens x 16 heads): split-f16 matrix-core kernel
        return 2
    return 0


ATTENTION_KERNELS = ("attn_fwd_kernel", "attn_short_kernel", "attn_x3_kernel", "attn_keysplit_kernel")      # DVIS_ATTN_* of dvis_hip.h
AttentionPlan = collections.namedtuple("AttentionPlan", "kernel nsplit keys_per_split qchunks")


def attention_plan(q, k, nheads, mask=None, short=False):
    """What ``attention(q, k, v, nheads, mask, short=short)`` would launch (v shaped and strided like k), without launching it:
    AttentionPlan(kernel, nsplit, keys_per_split, qchunks) — the kernel's name (ATTENTION_KERNELS), the number of key ranges whose
    partial results a second launch merges, the keys of each but the last (which holds Lk - (nsplit - 1) * keys_per_split) and the
    number of units along the queries (128 queries each on attn_fwd_kernel / attn_x3_kernel, 112 on attn_keysplit_kernel, 16 on
    attn_short_kernel).  The answer comes from dvis_attention_plan, the function the launch itself consults, after this module's
    own split-f16 rule; only shapes and strides are read, so CPU tensors are fine."""
    Lq, B, C = q.shape
    Lk = k.shape[0]
    d = C // nheads
    plan = (ctypes.c_int32 * 4)()
    rc = native.lib().dvis_attention_plan(B * nheads, Lq, Lk, d, int(mask is not None), k.stride(0), k.stride(0),
                                          _attention_kernel_arg(Lq, Lk, d, mask is not None, short), plan)
    native.check(rc, "dvis_attention_plan")
    return AttentionPlan(ATTENTION_KERNELS[plan[0]], plan[1], plan[2], plan[3])


def _attention_kernel(q, k, v, nheads, mask=None, allowed_count=None, out=None, short=False):
    Lq, B, C = q.shape
    Lk = k.shape[0]
    d = C // nheads
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 3 or t.stride(2) != 1:
            raise RuntimeError(f"attention: {name} must be a float32 GPU (L, B, C) tensor with a contiguous last dim")
    if k.shape != v.shape or k.shape[1:] != q.shape[1:]:
        raise RuntimeError("attention: inconsistent q / k / v shapes")
    if out is None:
        out = torch.empty((Lq, B, C), dtype=torch.float32, device=q.device)
    mptr = aptr = None
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        if mask.shape != (B, Lq, Lk) or mask.dtype != torch.uint8:
            raise RuntimeError("attention: mask must be uint8/bool (B, Lq, Lk)")
        mptr = native.dev_ptr(mask, "mask")
        if allowed_count is not None:
            if allowed_count.shape != (B, Lq) or allowed_count.dtype != torch.int32:
                raise RuntimeError("attention: allowed_count must be int32 (B, Lq)")
            aptr = native.dev_ptr(allowed_count, "allowed_count")
    lib = native.lib()
    kern = _attention_kernel_arg(Lq, Lk, d, mask is not None, short)
    if kern == 2:
        X3_GUARD.word(q.device)          # (its range guard reports under the tag of the last packed weight: the block's qkv)
    nbytes = lib.dvis_attention_ws_bytes_k(B * nheads, Lq, Lk, d, kern)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=q.device) if nbytes else None
    with torch.cuda.device(q.device):
        rc = lib.dvis_attention_forward_k(
            ctypes.c_void_p(q.data_ptr()), _strides3(q, B, C, d), ctypes.c_void_p(k.data_ptr()), _strides3(k, B, C, d),
            ctypes.c_void_p(v.data_ptr()), _strides3(v, B, C, d), ctypes.c_void_p(out.data_ptr()),
            _strides3(out, B, C, d), mptr, aptr, B, nheads, Lq, Lk, d, 1.0 / (d ** 0.5),
            ctypes.c_void_p(ws.data_ptr()) if ws is not None else None, native.stream_ptr(q.device), kern)
    native.check(rc, "dvis_attention_forward_k")
    return out


ATTENTION_BACKWARD_MAX_KEYS = 256
MASKED_ATTENTION_BACKWARD_MAX_QUERIES = 256
MASKED_ATTENTION_BACKWARD_MAX_KEYS = 65536
MaskedAttentionBackwardPlan = collections.namedtuple("MaskedAttentionBackwardPlan",
                                                     "key_tile query_tile n_key_tiles threads lds_bytes")


def _attention_grad_check(op, q, k, v, grad_out, nheads, out=None):
    """What csrc/attention_backward.hip and csrc/masked_attention_backward.hip both ask of their tensors, checked on the host before
    anything is launched; `op` names the caller in the messages."""
    tensors = [("q", q), ("k", k), ("v", v)] + [(n, t) for n, t in (("grad_out", grad_out), ("out", out)) if t is not None]
    for name, t in tensors:
        if not t.is_cuda or t.dim() != 3:
            raise RuntimeError(f"{op}: {name} must be a GPU (L, B, C) tensor")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{op}: {name} must be float32 (got {t.dtype})")
        if t.stride(2) != 1:
            raise RuntimeError(f"{op}: {name} must have inner stride 1 (got {t.stride(2)})")
    Lq, B, C = q.shape
    Lk = k.shape[0]
    if k.shape != v.shape or k.shape[1:] != q.shape[1:] or any(t is not None and t.shape != q.shape for t in (grad_out, out)):
        names = "q / k / v / grad_out" if op == "attention_backward" else "q / k / v / grad_out / out"      # (the first takes no out)
        raise RuntimeError(f"{op}: inconsistent {names} shapes")
    if C % nheads or C // nheads not in (32, 64):
        raise RuntimeError(f"{op}: head dim must be 32 or 64 (got C={C} over {nheads} heads)")
    if Lq < 1 or Lk < 1:
        raise RuntimeError(f"{op}: needs Lq >= 1 and Lk >= 1 (got Lq={Lq}, Lk={Lk})")


def _attention_backward_check(q, k, v, grad_out, nheads):
    """The contract of csrc/attention_backward.hip."""
    _attention_grad_check("attention_backward", q, k, v, grad_out, nheads)
    Lk = k.shape[0]
    if Lk > ATTENTION_BACKWARD_MAX_KEYS:
        raise RuntimeError(f"attention_backward: serves at most {ATTENTION_BACKWARD_MAX_KEYS} keys (got Lk={Lk})")


def _masked_attention_backward_check(q, k, v, grad_out, nheads, mask, allowed_count, out=None):
    """The contract of csrc/masked_attention_backward.hip.  Returns the mask as uint8."""
    _attention_grad_check("masked_attention_backward", q, k, v, grad_out, nheads, out)
    Lq, B, _ = q.shape
    Lk = k.shape[0]
    if Lq > MASKED_ATTENTION_BACKWARD_MAX_QUERIES:
        raise RuntimeError(f"masked_attention_backward: serves at most {MASKED_ATTENTION_BACKWARD_MAX_QUERIES} queries (got Lq={Lq})")
    if Lk > MASKED_ATTENTION_BACKWARD_MAX_KEYS:
        raise RuntimeError(f"masked_attention_backward: serves at most {MASKED_ATTENTION_BACKWARD_MAX_KEYS} keys (got Lk={Lk})")
    if mask is None:
        return None
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if mask.dtype != torch.uint8 or mask.shape != (B, Lq, Lk) or not mask.is_cuda:
        raise RuntimeError(f"masked_attention_backward: mask must be a uint8 / bool GPU tensor of shape (B, Lq, Lk) = {(B, Lq, Lk)} "
                           f"(got {mask.dtype} {tuple(mask.shape)})")
    if allowed_count is None:
        raise RuntimeError("masked_attention_backward: a mask needs its allowed_count (int32 (B, Lq), from attn_mask)")
    if allowed_count.dtype != torch.int32 or allowed_count.shape != (B, Lq) or not allowed_count.is_cuda:
        raise RuntimeError(f"masked_attention_backward: allowed_count must be an int32 GPU tensor of shape (B, Lq) = {(B, Lq)}")
    return mask


def _attention_grads_launch(q, k, v, grad_out, nheads, launch):
    """What attention_backward and masked_attention_backward do alike: allocate dq (Lq, B, C), dk and dv (Lk, B, C) and, unless
    B == 0, call ``launch(views, grads, sizes, dev)`` on q's device with the argument runs the library's two entry points share —
    the (pointer, strides) pairs of q, k, v, grad_out; the pointers of dq, dk, dv; (B, heads, Lq, Lk, d, scale).  `launch` returns the
    library's status and the entry point's name."""
    Lq, B, C = q.shape
    Lk = k.shape[0]
    d = C // nheads
    dev = q.device
    dq = torch.empty((Lq, B, C), dtype=torch.float32, device=dev)
    dk = torch.empty((Lk, B, C), dtype=torch.float32, device=dev)
    dv = torch.empty((Lk, B, C), dtype=torch.float32, device=dev)
    if B:
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        views = [a for t in (q, k, v, grad_out) for a in (ptr(t), _strides3(t, B, C, d))]
        with torch.cuda.device(dev):
            rc, what = launch(views, (ptr(dq), ptr(dk), ptr(dv)), (B, nheads, Lq, Lk, d, 1.0 / (d ** 0.5)), dev)
        native.check(rc, what)
    return dq, dk, dv


def attention_backward(q, k, v, grad_out, nheads):
    """Gradients of ``attention(q, k, v, nheads)`` (no mask) for the upstream gradient ``grad_out`` (csrc/attention_backward.hip):
    q / grad_out (Lq, B, C), k / v (Lk, B, C) float32 GPU tensors with unit inner stride and arbitrary row / batch strides, head dim
    32 or 64, Lk <= 256 -> (dq (Lq, B, C), dk (Lk, B, C), dv (Lk, B, C)), contiguous.  The probabilities are recomputed from q and
    k.  Exact fp32, no atomics: the same bits on every call, and a batch entry's bits do not depend on B.  Anything outside the
    contract raises before a launch; there is no torch formulation behind it for GPU tensors."""
    _attention_backward_check(q, k, v, grad_out, nheads)

    def launch(views, grads, sizes, dev):
        return native.lib().dvis_attention_backward(*views, *grads, *sizes, native.stream_ptr(dev)), "dvis_attention_backward"

    return _attention_grads_launch(q, k, v, grad_out, nheads, launch)


def attention_backward_threads(Lk):
    """Threads per workgroup ``attention_backward`` launches for Lk keys (64, 128 or 256: 4, 8 or 16 lanes per query row in the row
    reductions) — asked of the library, whose launch uses the same function."""
    n = native.lib().dvis_attention_backward_threads(int(Lk))
    if n <= 0:
        raise RuntimeError(f"attention_backward: serves 1 .. {ATTENTION_BACKWARD_MAX_KEYS} keys (got Lk={Lk})")
    return n


def masked_attention_backward_plan(Lq, Lk, d):
    """How ``masked_attention_backward`` cuts Lq queries and Lk keys of head dim d: MaskedAttentionBackwardPlan(key_tile, query_tile,
    n_key_tiles, threads, lds_bytes) — keys per workgroup, queries per chunk inside it, workgroups per (batch entry, head), threads per
    workgroup, dynamic LDS — asked of the library, whose launch uses the same function."""
    plan = (ctypes.c_int32 * 5)()
    native.check(native.lib().dvis_masked_attention_backward_plan(int(Lq), int(Lk), int(d), plan),
                 "dvis_masked_attention_backward_plan")
    return MaskedAttentionBackwardPlan(*plan)


def masked_attention_backward(q, k, v, grad_out, nheads, mask=None, allowed_count=None, out=None):
    """Gradients of ``masked_attention(q, k, v, nheads, mask, allowed_count)`` for the upstream gradient ``grad_out``
    (csrc/masked_attention_backward.hip): q / grad_out (Lq, B, C), k / v (Lk, B, C) float32 GPU tensors with unit inner stride and
    arbitrary row / batch strides, head dim 32 or 64, Lq <= 256, Lk <= 65536; mask uint8 / bool (B, Lq, Lk) with 1 = blocked and its
    allowed_count int32 (B, Lq) (a row with count 0 ignores its mask) -> (dq (Lq, B, C), dk (Lk, B, C), dv (Lk, B, C)), contiguous.
    ``out`` — the forward's result for the same arguments — is accepted and checked for its shape but not read: the kernel takes
    D = rowsum(P o dP) from the probabilities it recomputes (csrc/masked_attention_backward.hip says why), so no forward call is
    needed either.  A blocked key gets no contribution from the query that blocks it.  Exact fp32, no atomics:
    the same bits on every call, and a batch entry's bits do not depend on B.  Anything outside the contract raises before a
    launch; there is no torch formulation behind it for GPU tensors."""
    mask = _masked_attention_backward_check(q, k, v, grad_out, nheads, mask, allowed_count, out)

    def launch(views, grads, sizes, dev):
        lib = native.lib()
        B, heads, Lq, Lk, d, _ = sizes
        ws = torch.empty((lib.dvis_masked_attention_backward_ws_bytes(B * heads, Lq, Lk, d) // 4,), dtype=torch.float32, device=dev)
        return lib.dvis_masked_attention_backward(
            *views, native.dev_ptr(mask, "mask") if mask is not None else None,
            native.dev_ptr(allowed_count, "allowed_count") if mask is not None else None, *grads, *sizes,
            ctypes.c_void_p(ws.data_ptr()), native.stream_ptr(dev)), "dvis_masked_attention_backward"

    return _attention_grads_launch(q, k, v, grad_out, nheads, launch)


def _grad_out_for_kernel(grad_out):
    """The backward kernels' view contract: unit inner stride, 16-byte aligned base, row / batch strides in multiples of 4 floats.
    What autograd hands over need not meet it (the narrowed gradient of a concatenation, an odd stride on a dim of size 1): copy."""
    B = grad_out.shape[1]
    if grad_out.stride(2) != 1 or grad_out.data_ptr() % 16 or grad_out.stride(0) % 4 or (B > 1 and grad_out.stride(1) % 4):
        return grad_out.contiguous()
    return grad_out


class AttentionFunction(Function):
    """``attention`` (no mask) and ``masked_attention`` under autograd: the forward kernel as it is; for q, k and v
    csrc/attention_backward.hip (tiled=False) or csrc/masked_attention_backward.hip (tiled=True: a mask, long key sequences).  Which
    of the two is the caller's choice alone, never a function of Lk or of the mask; the mask and its counts get no gradient."""

    @staticmethod
    def forward(ctx, q, k, v, nheads, mask, allowed_count, short, tiled):
        ctx.save_for_backward(q, k, v, mask, allowed_count)       # (not the output: the backward recomputes what it needs)
        ctx.nheads, ctx.tiled = nheads, tiled
        return _attention_kernel(q, k, v, nheads, mask, allowed_count, short=short)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        q, k, v, mask, allowed_count = ctx.saved_tensors
        grad_out = _grad_out_for_kernel(grad_out)
        if ctx.tiled:
            dq, dk, dv = masked_attention_backward(q, k, v, grad_out, ctx.nheads, mask, allowed_count)
        else:
            dq, dk, dv = attention_backward(q, k, v, grad_out, ctx.nheads)
        need = ctx.needs_input_grad
        return dq if need[0] else None, dk if need[1] else None, dv if need[2] else None, None, None, None, None, None


MaskedAttentionFunction = AttentionFunction       # (the name DESIGN.md and CHANGELOG.md know masked_attention's wiring by)


def masked_attention(q, k, v, nheads, mask=None, allowed_count=None):
    """``attention(q, k, v, nheads, mask, allowed_count)`` — the same forward kernel, the same bits — that is differentiable WITH a
    mask and over long key sequences: an input that requires grad routes the call through AttentionFunction (tiled=True: backward
    csrc/masked_attention_backward.hip: Lq <= 256, Lk <= 65536, head dim 32 or 64; a mask needs its allowed_count).  The
    cross-attention of the masked-attention decoder in training.  CPU tensors: cpu_ops.attention and torch's own autograd."""
    if _on_cpu(q, k, v):
        return cpu_ops.attention(q, k, v, nheads, mask, allowed_count)
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        mask = _masked_attention_backward_check(q, k, v, None, nheads, mask, allowed_count)
        return AttentionFunction.apply(q, k, v, nheads, mask, allowed_count, False, True)
    return _attention_kernel(q, k, v, nheads, mask, allowed_count)


def window_attention_supported(ws, d):
    """Whether csrc/window_attention.hip serves window size `ws` at head dim `d` (asked of the library itself)."""
    return bool(native.lib().dvis_window_attention_supported(int(ws), int(d)))


def window_attention(qkv, qkv_bias, bias_table, B, H, W, heads, ws, shift, scale=None, out=None):
    """Swin's shifted-window attention on the block's qkv projection (swin.py:131-171, 235-295, 413-440): pad, cyclic shift, window
    partition, per-head relative-position bias, region mask, softmax, P V, window reverse, reverse shift and crop in ONE kernel
    (csrc/window_attention.hip; the contract is spelled out at dvis_window_attention in include/dvis_hip.h).
    qkv (B, H W, 3 C) on the UNPADDED token grid, columns [3][heads][d]; qkv_bias (3 C) or None: what a pad token's q / k / v is (the
    reference pads after norm1); bias_table ((2 ws - 1)^2, heads), raw; 0 <= shift < ws; scale defaults to d^-0.5.
    -> (B, H W, C), columns [heads][d], ready for the out-projection (written into `out`, a contiguous fp32 GPU tensor of that shape,
    when given: every row of it is written).
    fp32 contiguous GPU tensors run the kernel; a (ws, d) it does not serve raises (DVIS_STRICT=0: cpu_ops.window_attention's torch
    formulation on the GPU).  CPU tensors (any float dtype) take cpu_ops.window_attention.  There is no backward: an input that
    requires grad on the GPU raises."""
    tensors = [t for t in (qkv, qkv_bias, bias_table) if t is not None]
    C = qkv.shape[-1] // 3
    d = C // heads
    if qkv.dim() != 3 or tuple(qkv.shape) != (B, H * W, 3 * heads * d) or tuple(bias_table.shape) != ((2 * ws - 1) ** 2, heads) \
            or (qkv_bias is not None and tuple(qkv_bias.shape) != (3 * C,)) or not 0 <= shift < ws:
        raise RuntimeError(f"window_attention: expected qkv (B, H W, 3 heads d), qkv_bias (3 C), bias_table ((2 ws - 1)^2, heads) and "
                           f"0 <= shift < ws; got qkv {tuple(qkv.shape)}, bias_table {tuple(bias_table.shape)}, B={B} H={H} W={W} "
                           f"heads={heads} ws={ws} shift={shift}")
    if _on_cpu(*tensors):
        return cpu_ops.window_attention(qkv, qkv_bias, bias_table, B, H, W, heads, ws, shift, scale)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError("window_attention: there is no window-attention backward (csrc/window_attention.hip is inference-only); "
                           "call it under torch.no_grad() or detach qkv, qkv_bias and bias_table")
    for name, t in (("qkv", qkv), ("qkv_bias", qkv_bias), ("bias_table", bias_table)):
        if t is not None and not (t.is_cuda and t.device == qkv.device and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError(f"window_attention: {name} must be a contiguous float32 tensor on qkv's GPU (got {t.dtype} on {t.device}, "
                               f"contiguous {t.is_contiguous()})")
    scale = float(d ** -0.5 if scale is None else scale)
    if not window_attention_supported(ws, d):
        _torch_path("window_attention", qkv, f"the kernel does not serve window size ws={ws} with head dim d={d}: d=32 with ws=7 or ws=12")
        return cpu_ops.window_attention(qkv, qkv_bias, bias_table, B, H, W, heads, ws, shift, scale)
    if out is None:
        out = torch.empty((B, H * W, C), dtype=torch.float32, device=qkv.device)
    elif tuple(out.shape) != (B, H * W, C) or out.dtype != torch.float32 or out.device != qkv.device:
        raise RuntimeError(f"window_attention: out must be float32 {(B, H * W, C)} on qkv's GPU")
    with torch.cuda.device(qkv.device):
        rc = native.lib().dvis_window_attention(native.dev_ptr(qkv, "qkv"), None if qkv_bias is None else native.dev_ptr(qkv_bias, "qkv_bias"),
                                                native.dev_ptr(bias_table, "bias_table"), native.dev_ptr(out, "out"), B, H, W, heads, d, ws,
                                                shift, scale, native.stream_ptr(qkv.device))
    native.check(rc, "dvis_window_attention")
    return out


# ---- first half of a ConvNeXt block: csrc/dwconv_ln.hip ---------------------------------------------------------------------------
def _dwconv7x7_ln_shape(x, hw):
    """(B, h, w, C) of the token-major map: x (B, h, w, C), or x (B, h w, C) with hw = (h, w)."""
    if x.dim() == 4 and hw is None:
        return tuple(x.shape)
    if x.dim() == 3 and hw is not None and int(hw[0]) * int(hw[1]) == x.shape[1]:
        return x.shape[0], int(hw[0]), int(hw[1]), x.shape[2]
    raise RuntimeError(f"dwconv7x7_ln_tokens: expected x (B, h, w, C), or x (B, h w, C) with hw=(h, w); got {tuple(x.shape)} and hw={hw}")


def dwconv7x7_ln_tokens_ok(x, conv_dw, norm, hw=None):
    """Whether ``dwconv7x7_ln_tokens`` runs csrc/dwconv_ln.hip on these operands: float32 GPU tensors on one device, a depthwise
    7 x 7 / stride 1 / padding 3 convolution, an affine LayerNorm over C, and a width the library serves (asked of the library
    itself: C % 4 == 0, 8 <= C <= 1536) with one frame below 2^31 bytes."""
    B, h, w, C = _dwconv7x7_ln_shape(x, hw)
    tensors = [x, conv_dw.weight, conv_dw.bias, norm.weight, norm.bias]
    return (all(t is None or (t.is_cuda and t.device == x.device and t.dtype == torch.float32) for t in tensors)
            and norm.weight is not None and norm.bias is not None and tuple(conv_dw.weight.shape) == (C, 1, 7, 7)
            and tuple(norm.weight.shape) == (C,) and tuple(conv_dw.stride) == (1, 1) and tuple(conv_dw.padding) == (3, 3)
            and tuple(conv_dw.dilation) == (1, 1) and conv_dw.groups == C and h * w * C * 4 < 2 ** 31
            and bool(native.lib().dvis_dwconv7x7_ln_tokens_supported(int(C))))


def dwconv7x7_ln_tokens(x, conv_dw, norm, hw=None, out=None):
    """``norm(conv_dw(x_nchw).permute(0, 2, 3, 1))`` of a ConvNeXt block — depthwise 7 x 7 convolution + bias, then LayerNorm over the
    channels — on the TOKEN-major map, in one kernel (csrc/dwconv_ln.hip; contract: dvis_dwconv7x7_ln_tokens in include/dvis_hip.h).
    x (B, h, w, C), or (B, h w, C) with hw = (h, w); a view whose frames are contiguous (h w C) blocks at a batch stride that is a
    multiple of 4 floats is read in place.  conv_dw: an ``nn.Conv2d(C, C, 7, padding=3, groups=C)`` (bias optional); norm: an affine
    ``nn.LayerNorm(C)``.  -> a new contiguous tensor of x's shape (or `out`, a contiguous float32 GPU tensor of that shape that does
    not overlap x: every element of it is written).
    Exact fp32, a fixed operation order: the same bits every call, and a frame's bits do not depend on B.  Operands the kernel does
    not serve (``dwconv7x7_ln_tokens_ok``) raise (DVIS_STRICT=0: cpu_ops.dwconv7x7_ln_tokens' torch formulation on the GPU).  CPU
    tensors (any float dtype) take cpu_ops.dwconv7x7_ln_tokens.  No backward on the GPU: the trunk is frozen in every config."""
    B, h, w, C = _dwconv7x7_ln_shape(x, hw)
    tensors = [x, conv_dw.weight, conv_dw.bias, norm.weight, norm.bias]
    if _on_cpu(*[t for t in tensors if t is not None]):
        return cpu_ops.dwconv7x7_ln_tokens(x, conv_dw, norm, hw)
    _no_backward("dwconv7x7_ln_tokens", tensors)
    if not dwconv7x7_ln_tokens_ok(x, conv_dw, norm, hw):
        _torch_path("dwconv7x7_ln_tokens", x, f"needs float32 tensors on one GPU, a depthwise 7 x 7 / stride 1 / padding 3 convolution "
                    f"and an affine LayerNorm over C % 4 == 0, 8 <= C <= 1536, one frame below 2^31 bytes (C={C}, frame h w C * 4 = "
                    f"{h * w * C * 4} bytes)")
        return cpu_ops.dwconv7x7_ln_tokens(x, conv_dw, norm, hw)
    frame = h * w * C
    xs = x.detach()
    in_place = xs.data_ptr() % 16 == 0 and (B == 0 or (xs[0].is_contiguous()
                                                       and (B == 1 or (xs.stride(0) % 4 == 0 and xs.stride(0) >= frame))))
    if not in_place:
        xs = xs.contiguous()
    bstride = xs.stride(0) if B > 1 else frame
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    elif out.shape != x.shape or out.dtype != torch.float32 or out.device != x.device:
        raise RuntimeError(f"dwconv7x7_ln_tokens: out must be float32 {tuple(x.shape)} on x's GPU")
    wt = conv_dw.weight.detach().contiguous()
    bias = None if conv_dw.bias is None else native.dev_ptr(conv_dw.bias.detach().contiguous(), "bias")
    with torch.cuda.device(x.device):
        rc = native.lib().dvis_dwconv7x7_ln_tokens(ctypes.c_void_p(xs.data_ptr()), native.dev_ptr(out, "out"), bstride, B, h, w, C,
                                                   native.dev_ptr(wt, "weight"), bias, native.dev_ptr(norm.weight.detach(), "gamma"),
                                                   native.dev_ptr(norm.bias.detach(), "beta"), float(norm.eps),
                                                   native.stream_ptr(x.device))
    native.check(rc, "dvis_dwconv7x7_ln_tokens")
    return out


# ---- classification of the open-vocabulary (FC-CLIP) heads: csrc/mask_pool.hip, csrc/ov_class_logits.hip ----------------------------
MaskPoolPlan = collections.namedtuple("MaskPoolPlan", "slab slabs")


def _no_backward(op, tensors):
    """The open-vocabulary ops are inference-only on the GPU: an input that requires grad with grad enabled raises, naming the op."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(f"{op}: there is no backward for {op} on the GPU (the open-vocabulary kernels are inference-only); call it "
                           "under torch.no_grad() or detach its inputs")


def mask_pool_plan(B, Q, C, H, W):
    """How csrc/mask_pool.hip would pool x (B, C, H, W) under mask logits (B, Q, H, W), without launching it: MaskPoolPlan(slab,
    slabs) — the pixels of one slab and the number of slabs whose partial sums are added in order, a function of H W alone.  Asked
    of the library (dvis_mask_pool_plan, which applies the served-shape checks of the call itself: Q <= 256, C % 4 == 0 up to 2048,
    frames below 2^31 bytes); a shape it does not serve raises, naming the value.  Only sizes are read: no GPU is needed."""
    plan = (ctypes.c_int32 * 2)()
    native.check(native.lib().dvis_mask_pool_plan(int(B), int(Q), int(C), int(H) * int(W), plan), "dvis_mask_pool_plan")
    return MaskPoolPlan(plan[0], plan[1])


def mask_pool(x, mask_logits):
    """The sums and pixel counts of MaskPooling (ov_dvis/video_mask2former_transformer_decoder_ov.py:39-67): x (B, C, H, W) and
    mask_logits (B, Q, H, W) -> (sum (B, Q, C) of x over the pixels with logit > 0, count (B, Q) int32 of those pixels).  0.0, -0.0
    and NaN logits are outside the mask.  The mean is ``mask_pool_mean``; sums and counts come separately because the refiner
    combines frames by their pixel counts.
    GPU: csrc/mask_pool.hip (contract: dvis_mask_pool in include/dvis_hip.h) on float32 tensors, x contiguous; mask_logits may be any
    view whose (H, W) planes are contiguous — a frame ``logits[0, :, t]`` of the (1, Q, T, H, W) inference logits is read in place.
    Exact fp32, no atomics: the same bits on every call, and a frame's bits do not depend on B.  A shape outside the served domain
    (``mask_pool_plan``) raises.  CPU tensors (any float dtype) take cpu_ops.mask_pool.  No backward on the GPU."""
    if x.dim() != 4 or mask_logits.dim() != 4 or x.shape[0] != mask_logits.shape[0] or x.shape[-2:] != mask_logits.shape[-2:]:
        raise RuntimeError(f"mask_pool: expected x (B, C, H, W) and mask_logits (B, Q, H, W) on one map size; got {tuple(x.shape)} and "
                           f"{tuple(mask_logits.shape)} (MaskPooling interpolates differing sizes before it pools)")
    if _on_cpu(x, mask_logits):
        return cpu_ops.mask_pool(x, mask_logits)
    _no_backward("mask_pool", (x, mask_logits))
    B, C, H, W = x.shape
    Q = mask_logits.shape[1]
    px = _f32_gpu(x, "x")
    if not (mask_logits.is_cuda and mask_logits.device == x.device and mask_logits.dtype == torch.float32):
        raise RuntimeError(f"mask_pool: mask_logits must be a float32 tensor on x's GPU (got {mask_logits.dtype} on {mask_logits.device})")
    if H * W > 1 and not ((W == 1 or mask_logits.stride(3) == 1) and (H == 1 or mask_logits.stride(2) == W)):
        raise RuntimeError(f"mask_pool: the (H, W) planes of mask_logits must be contiguous (got strides {mask_logits.stride()})")
    dev = x.device
    total = torch.empty((B, Q, C), dtype=torch.float32, device=dev)
    count = torch.empty((B, Q), dtype=torch.int32, device=dev)
    lib = native.lib()
    nbytes = lib.dvis_mask_pool_ws_bytes(B, Q, C, H * W)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        rc = lib.dvis_mask_pool(px, ctypes.c_void_p(mask_logits.data_ptr()), mask_logits.stride(0) if B > 1 else 0,
                                mask_logits.stride(1) if Q > 1 else H * W, B, Q, C, H * W, native.dev_ptr(total, "sum"),
                                native.dev_ptr(count, "count"), ctypes.c_void_p(ws.data_ptr()) if ws is not None else None,
                                native.stream_ptr(dev))
    native.check(rc, "dvis_mask_pool")
    return total, count


def mask_pool_mean(x, mask_logits):
    """MaskPooling.forward(x, mask, return_num=True): (pooled (B, Q, C) = sum / (count + 1e-8), denorm (B, Q, 1, 1) = count + 1e-8),
    computed as the reference does — a row without a pixel pools to exactly 0."""
    total, count = mask_pool(x, mask_logits)
    denorm = count.to(total.dtype) + 1e-8
    return total / denorm.unsqueeze(-1), denorm[..., None, None]


_seg_ptr_cache = {}


def _seg_ptr(num_templates, N, device):
    """Device int32 prefix sums of num_templates (K + 2 entries), cached per (device, tuple).  An inconsistent list raises."""
    key = tuple(int(n) for n in num_templates)
    if not key or min(key) < 1 or sum(key) != N:
        raise RuntimeError(f"text_class_logits: num_templates must list at least one template per group (the void group last) and add "
                           f"up to the {N} rows of text_classifier; got {len(key)} groups adding up to {sum(key)}"
                           + (f", smallest {min(key)}" if key else ""))
    hit = _seg_ptr_cache.get((str(device), key))
    if hit is None:
        hit = _seg_ptr_cache[(str(device), key)] = torch.tensor([0, *key], dtype=torch.int64).cumsum(0).to(torch.int32).to(device)
    return hit


def text_class_logits(x, text_classifier, logit_scale, num_templates):
    """get_classification_logits (ov_dvis/video_mask2former_transformer_decoder_ov.py:17-36): x (..., D), text_classifier (N, D),
    logit_scale a 0-d tensor (a parameter: read on the device, no synchronisation), num_templates the templates per class with the
    void group last -> (..., K + 1) = max over a group's templates of min(exp(logit_scale), 100) * normalize(x) @ text^T.
    num_templates must add up to N with no empty group (the reference silently takes "the last n rows" for the void group; with a
    consistent list the two agree).
    GPU, float32: the products on the exact-fp32 GEMM (gemm_nt on the raw x; D % 4 == 0), then ONE epilogue launch for the row
    norm, the scale and the segmented maximum (csrc/ov_class_logits.hip).  CPU tensors (any float dtype): cpu_ops.  No backward on
    the GPU."""
    N, D = text_classifier.shape
    if x.shape[-1] != D or not torch.is_tensor(logit_scale) or logit_scale.numel() != 1:
        raise RuntimeError(f"text_class_logits: expected x (..., D), text_classifier (N, D) and a one-element logit_scale tensor; got "
                           f"{tuple(x.shape)}, {tuple(text_classifier.shape)}")
    seg = _seg_ptr(num_templates, N, x.device)
    if _on_cpu(x, text_classifier, logit_scale):
        return cpu_ops.text_class_logits(x, text_classifier, logit_scale, num_templates)
    _no_backward("text_class_logits", (x, text_classifier, logit_scale))
    for name, t in (("x", x), ("text_classifier", text_classifier), ("logit_scale", logit_scale)):
        if not (t.is_cuda and t.device == x.device and t.dtype == torch.float32):
            raise RuntimeError(f"text_class_logits: {name} must be a float32 tensor on x's GPU (got {t.dtype} on {t.device})")
    x2, ldx = _rows2d(x.detach(), D)
    dots = gemm_nt(x2, text_classifier.detach())                                                # (R, N)
    R, K1 = x2.shape[0], seg.numel() - 1
    out = torch.empty((*x.shape[:-1], K1), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = native.lib().dvis_text_class_logits(ctypes.c_void_p(x2.data_ptr()), ldx, native.dev_ptr(dots, "dots"), N,
                                                 ctypes.c_void_p(logit_scale.data_ptr()), native.dev_ptr(seg, "seg_ptr"), R, D, N, K1,
                                                 native.dev_ptr(out, "out"), native.stream_ptr(x.device))
    native.check(rc, "dvis_text_class_logits")
    return out


def ov_ensemble(in_logits, out_logits, overlapping, alpha, beta, valid=None):
    """The geometric ensemble of the open-vocabulary meta-architectures (ov_dvis/meta_architecture_ov.py:603-642) in one launch
    (contract: dvis_ov_ensemble in include/dvis_hip.h): in_logits / out_logits (..., K + 1) in- / out-vocabulary class logits with
    void last, overlapping (K) non-zero where the category was seen in training (alpha there, beta elsewhere), valid (...) integer
    pixel counts or None (ENSEMBLE_ON_VALID_MASK: rows with valid <= 0 keep the in-vocabulary distribution) ->
    log(cat(softmax(c) (1 - p_void), p_void) + 1e-8), evaluated in the log domain.  GPU: float32, K <= 2048.  CPU tensors (any float
    dtype): cpu_ops.ov_ensemble.  No backward on the GPU."""
    K = in_logits.shape[-1] - 1
    if in_logits.shape != out_logits.shape or K < 1 or overlapping.numel() != K \
            or (valid is not None and tuple(valid.shape) != tuple(in_logits.shape[:-1])):
        raise RuntimeError(f"ov_ensemble: expected in_logits and out_logits (..., K + 1), overlapping (K) and valid (...); got "
                           f"{tuple(in_logits.shape)}, {tuple(out_logits.shape)}, {tuple(overlapping.shape)}"
                           + ("" if valid is None else f", {tuple(valid.shape)}"))
    if _on_cpu(in_logits, out_logits):
        return cpu_ops.ov_ensemble(in_logits, out_logits, overlapping.reshape(K), alpha, beta, valid)
    _no_backward("ov_ensemble", (in_logits, out_logits))
    dev = in_logits.device
    for name, t in (("in_logits", in_logits), ("out_logits", out_logits)):
        if not (t.is_cuda and t.device == dev and t.dtype == torch.float32):
            raise RuntimeError(f"ov_ensemble: {name} must be a float32 tensor on in_logits' GPU (got {t.dtype} on {t.device})")
    a, b = in_logits.contiguous(), out_logits.contiguous()
    ov = overlapping.reshape(K).to(device=dev, dtype=torch.float32).contiguous()
    vp = None
    if valid is not None:
        valid = valid.to(device=dev, dtype=torch.int32).contiguous()
        vp = native.dev_ptr(valid, "valid")
    out = torch.empty_like(a)
    with torch.cuda.device(dev):
        rc = native.lib().dvis_ov_ensemble(native.dev_ptr(a, "in_logits"), native.dev_ptr(b, "out_logits"), native.dev_ptr(ov, "overlapping"),
                                           vp, float(alpha), float(beta), a.numel() // (K + 1), K, native.dev_ptr(out, "out"),
                                           native.stream_ptr(dev))
    native.check(rc, "dvis_ov_ensemble")
    return out


POSTPROCESS_OPS = ("vps_argmax", "vss_argmax", "resize2", "resize2_gt0")                   # DVIS_POST_* of dvis_hip.h
PostprocessPlan = collections.namedtuple("PostprocessPlan", "workgroups sweeps form K4 identity lds_bytes row_stride")


def vss_row_stride(C):
    """Floats per row of the zero-padded class matrix that ``vss_argmax`` hands to dvis_vss_argmax: C rounded up to 32."""
    return (int(C) + 31) // 32 * 32


def postprocess_plan(op, K, T, img_size, out_hw, C=None):
    """How csrc/postprocess.hip would run ``vps_argmax`` / ``vss_argmax`` / ``resize2`` / ``resize2_gt0`` (`op`, one of
    POSTPROCESS_OPS) on K candidate maps (vss_argmax: K queries and C classes) of T frames, without launching it:
    PostprocessPlan(workgroups, sweeps, form, K4, identity, lds_bytes, row_stride) — the workgroups launched and the grid-stride
    sweeps they make (0, 0: nothing is launched); for vss_argmax also the form ("mfma" or "generic"), K4 (float4 of class sums per
    thread: the generic form's instance), whether the second resize is the identity, the dynamic LDS bytes and the class matrix's row
    stride (``vss_row_stride``); None / 0 / False for the other ops.  The answer comes from dvis_postprocess_plan, the function the
    launches themselves consult; only sizes are read, so no GPU is needed.  A size the call refuses raises with the call's message."""
    code = POSTPROCESS_OPS.index(op)
    vss = op == "vss_argmax"
    if vss == (C is None):
        raise RuntimeError("postprocess_plan: C is the class count of vss_argmax (and of nothing else)")
    stride = vss_row_stride(C) if vss else 0
    plan = (ctypes.c_int32 * 6)()
    rc = native.lib().dvis_postprocess_plan(code, int(K), int(C) if vss else 0, stride, int(T), int(img_size[0]), int(img_size[1]),
                                            int(out_hw[0]), int(out_hw[1]), plan)
    native.check(rc, "dvis_postprocess_plan")
    if not vss:
        return PostprocessPlan(plan[0], plan[1], None, 0, False, 0, 0)
    return PostprocessPlan(plan[0], plan[1], "mfma" if plan[2] else "generic", plan[3], bool(plan[4]), plan[5], stride)


def vps_argmax(mask_logits_kthw, scores, first_resize_size, img_size, out_hw):
    """Fused panoptic arg-max (see dvis_vps_argmax).  mask_logits_kthw: float32 GPU (K, T, h, w) view whose last two
    dims are contiguous; scores float32 (K,).  Returns ids int32 (T,H,W), conf bool (T,H,W), areas int32 (3, K)."""
    K, T, h, w = mask_logits_kthw.shape
    m = mask_logits_kthw
    if not m.is_cuda or m.dtype != torch.float32 or m.stride(3) != 1 or m.stride(2) != w:
        raise RuntimeError("vps_argmax: logits must be a float32 GPU (K, T, h, w) view with contiguous (h, w) maps")
    scores = scores.to(torch.float32).contiguous()
    oh, ow = int(out_hw[0]), int(out_hw[1])
    ids = torch.empty((T, oh, ow), dtype=torch.int32, device=m.device)
    conf = torch.empty((T, oh, ow), dtype=torch.uint8, device=m.device)
    areas = torch.empty((3, K), dtype=torch.int32, device=m.device)
    with torch.cuda.device(m.device):
        rc = native.lib().dvis_vps_argmax(
            ctypes.c_void_p(m.data_ptr()), m.stride(0), m.stride(1), native.dev_ptr(scores, "scores"), K, T, h, w,
            int(first_resize_size[0]), int(first_resize_size[1]), int(img_size[0]), int(img_size[1]), oh, ow,
            native.dev_ptr(ids, "ids"), native.dev_ptr(conf, "conf"), native.dev_ptr(areas, "areas"),
            native.stream_ptr(m.device))
    native.check(rc, "dvis_vps_argmax")
    return ids, conf.bool(), areas


def resize2_gt0(mask_logits_kthw, first_resize_size, img_size, out_hw):
    """``F.interpolate(F.interpolate(m, first)[:, :, :img_h, :img_w], out_hw) > 0`` in one pass (see dvis_resize2_gt0):
    the instance masks of inference_video_vis.  m: float32 GPU (K, T, h, w) view with contiguous (h, w) maps.
    Returns bool (K, T, H, W)."""
    K, T, h, w = mask_logits_kthw.shape
    m = mask_logits_kthw
    if not m.is_cuda or m.dtype != torch.float32 or m.stride(3) != 1 or m.stride(2) != w:
        raise RuntimeError("resize2_gt0: logits must be a float32 GPU (K, T, h, w) view with contiguous (h, w) maps")
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((K, T, oh, ow), dtype=torch.uint8, device=m.device)
    with torch.cuda.device(m.device):
        rc = native.lib().dvis_resize2_gt0(
            ctypes.c_void_p(m.data_ptr()), m.stride(0), m.stride(1), K, T, h, w, int(first_resize_size[0]),
            int(first_resize_size[1]), int(img_size[0]), int(img_size[1]), oh, ow, native.dev_ptr(out, "out"),
            native.stream_ptr(m.device))
    native.check(rc, "dvis_resize2_gt0")
    return out.view(torch.bool)


def resize2(mask_logits_kthw, first_resize_size, img_size, out_hw, sigmoid=False):
    """``F.interpolate(f(F.interpolate(m, first)[:, :, :img_h, :img_w]), out_hw)``, f = sigmoid or identity, in one pass and
    in torch's CPU operation order (see dvis_resize2).  Returns float32 (K, T, H, W)."""
    K, T, h, w = mask_logits_kthw.shape
    m = mask_logits_kthw
    if not m.is_cuda or m.dtype != torch.float32 or m.stride(3) != 1 or m.stride(2) != w:
        raise RuntimeError("resize2: logits must be a float32 GPU (K, T, h, w) view with contiguous (h, w) maps")
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((K, T, oh, ow), dtype=torch.float32, device=m.device)
    with torch.cuda.device(m.device):
        rc = native.lib().dvis_resize2(
            ctypes.c_void_p(m.data_ptr()), m.stride(0), m.stride(1), K, T, h, w, int(first_resize_size[0]),
            int(first_resize_size[1]), int(img_size[0]), int(img_size[1]), oh, ow, 1 if sigmoid else 0,
            native.dev_ptr(out, "out"), native.stream_ptr(m.device))
    native.check(rc, "dvis_resize2")
    return out


def vss_argmax(mask_logits_qthw, mask_cls, first_resize_size, img_size, out_hw):
    """Fused semantic arg-max (see dvis_vss_argmax).  mask_logits_qthw: float32 GPU (Q, T, h, w) view whose last two dims
    are contiguous; mask_cls float32 (Q, C), C <= 128.  Returns int64 (T, H, W) class indices."""
    Q, T, h, w = mask_logits_qthw.shape
    m = mask_logits_qthw
    if not m.is_cuda or m.dtype != torch.float32 or m.stride(3) != 1 or m.stride(2) != w:
        raise RuntimeError("vss_argmax: logits must be a float32 GPU (Q, T, h, w) view with contiguous (h, w) maps")
    C = mask_cls.shape[1]
    Cp = vss_row_stride(C)
    cls = torch.nn.functional.pad(mask_cls.to(torch.float32), (0, Cp - C)).contiguous()     # zero columns: never the max
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((T, oh, ow), dtype=torch.int64, device=m.device)
    with torch.cuda.device(m.device):
        rc = native.lib().dvis_vss_argmax(
            ctypes.c_void_p(m.data_ptr()), m.stride(0), m.stride(1), native.dev_ptr(cls, "mask_cls"), Cp, Q, C, T,
            h, w, int(first_resize_size[0]), int(first_resize_size[1]), int(img_size[0]), int(img_size[1]), oh, ow,
            native.dev_ptr(out, "out"), native.stream_ptr(m.device))
    native.check(rc, "dvis_vss_argmax")
    return out


def add_layer_norm(x, res, norm, pos=None):
    """``norm(x + res)`` for an ``nn.LayerNorm`` `norm` in ONE pass.  x contiguous float32 GPU (..., C); res: None or a
    tensor broadcast-free of x's shape whose rows (last dim) are contiguous.  CPU tensors / other dtypes use torch ops
    (library code, not one of the named hot ops).
    pos: optional (1, S, C) / (S, C) position embedding for x of shape (N, S, C): returns ``(out, out + pos)`` — the
    second tensor (the next encoder layer's query) is written by the same kernel."""
    C = x.shape[-1]

    def with_pos(out):
        return out if pos is None else (out, out + pos.reshape(1, -1, C))
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and C % 4 == 0 and C <= 1024
            and norm.weight is not None and not torch.is_grad_enabled()):
        _torch_path("add_layer_norm", x, "needs contiguous fp32 rows with C % 4 == 0, C <= 1024 and an affine norm")
        return with_pos(norm(x if res is None else x + res))
    rp, rs = None, 0
    if res is not None:
        if res.shape != x.shape or res.dtype != torch.float32 or not res.is_cuda:
            _torch_path("add_layer_norm", x, "residual must be fp32 of x's shape")
            return with_pos(norm(x + res))
        if not res.is_contiguous():
            res = res.contiguous()
        rp, rs = ctypes.c_void_p(res.data_ptr()), C
    out = torch.empty_like(x)
    rows = x.numel() // C
    pp, pos_rows, out_pos = None, 0, None
    if pos is not None:
        pos_rows = pos.numel() // C
        if x.dim() != 3 or x.shape[1] != pos_rows or pos.dtype != torch.float32 or not pos.is_cuda:
            raise RuntimeError("add_layer_norm: pos must be a float32 GPU (S, C) embedding for x of shape (N, S, C)")
        pos = pos.contiguous()
        pp, out_pos = native.dev_ptr(pos, "pos"), torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = native.lib().dvis_add_layernorm(
            ctypes.c_void_p(x.data_ptr()), rp, rs, native.dev_ptr(norm.weight, "gamma"), native.dev_ptr(norm.bias, "beta"),
            ctypes.c_void_p(out.data_ptr()), pp, pos_rows, None if pos is None else ctypes.c_void_p(out_pos.data_ptr()),
            rows, C, float(norm.eps), native.stream_ptr(x.device))
    native.check(rc, "dvis_add_layernorm")
    return out if pos is None else (out, out_pos)


def layer_norm(x, norm):
    """``norm(x)`` for an ``nn.LayerNorm`` over the last dim: the fused kernel where it serves the width (C <= 1024, C % 4 == 0),
    torch's LayerNorm beyond (the 1536 / 3072-wide norms of Swin-L and of the large CLIP ConvNeXt's head)."""
    if x.shape[-1] <= 1024 and x.shape[-1] % 4 == 0:
        return add_layer_norm(x.contiguous(), None, norm)
    return norm(x)


def bias_relu_maxpool(x, bias=None):
    """``F.max_pool2d(relu(x + bias[c]), 3, stride=2, padding=1)`` in one pass (the ResNet stem after its convolution):
    relu(max(x) + b), bit-identical because fp32 add and ReLU are monotonic.  Non-GPU / odd shapes use the torch ops."""
    N, C, H, W = x.shape
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and H % 2 == 0 and W % 8 == 0
            and not torch.is_grad_enabled()):
        _torch_path("bias_relu_maxpool", x, "needs contiguous fp32 NCHW with H % 2 == 0 and W % 8 == 0")
        import torch.nn.functional as F
        if bias is not None:
            x = x + bias.view(1, -1, 1, 1)
        return F.max_pool2d(torch.relu(x), kernel_size=3, stride=2, padding=1)
    out = torch.empty((N, C, H // 2, W // 2), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = native.lib().dvis_bias_relu_maxpool(native.dev_ptr(x, "x"),
                                                 None if bias is None else native.dev_ptr(bias, "bias"),
                                                 native.dev_ptr(out, "out"), N * C, C, H, W, native.stream_ptr(x.device))
    native.check(rc, "dvis_bias_relu_maxpool")
    return out


def _fused_map_ok(x):
    """fp32 NCHW GPU map outside autograd: the fused glue kernels apply; anything else takes the torch ops."""
    return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and not torch.is_grad_enabled()


def group_norm_affine(x, norm):
    """Statistics of ``nn.GroupNorm`` `norm` on x (N,C,H,W) in one read, as the per-plane affine (scale, shift), each
    (N*C,), with  norm(x)[n, c] == x[n, c] * scale[n*C + c] + shift[n*C + c].  None when the fused path does not apply
    (caller falls back to ``norm(x)``)."""
    N, C, H, W = x.shape
    G = norm.num_groups
    if not (_fused_map_ok(x) and C // G <= 1024):
        _torch_path("group_norm_affine", x, "needs contiguous fp32 NCHW, at most 1024 channels per group")
        return None
    scale = torch.empty(N * C, dtype=torch.float32, device=x.device)
    shift = torch.empty(N * C, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = native.lib().dvis_group_norm_affine(
            native.dev_ptr(x, "x"), None if norm.weight is None else native.dev_ptr(norm.weight.detach(), "gamma"),
            None if norm.bias is None else native.dev_ptr(norm.bias.detach(), "beta"), native.dev_ptr(scale, "scale"),
            native.dev_ptr(shift, "shift"), N, C, G, H * W, float(norm.eps), native.stream_ptr(x.device))
    native.check(rc, "dvis_group_norm_affine")
    return scale, shift


def scale_shift_act_(x, scale, shift, relu=False):
    """In place: x[n, c] = relu?(x[n, c] * scale[n*C + c] + shift[n*C + c]) on an fp32 NCHW GPU map."""
    N, C, H, W = x.shape
    with torch.cuda.device(x.device):
        rc = native.lib().dvis_scale_shift_act(native.dev_ptr(x, "x"), native.dev_ptr(scale, "scale"),
                                               native.dev_ptr(shift, "shift"), N * C, H * W, 1 if relu else 0,
                                               native.stream_ptr(x.device))
    native.check(rc, "dvis_scale_shift_act")
    return x


def upsample_add(lateral, top, lat_affine=None):
    """``lateral + F.interpolate(top, size=lateral.shape[-2:], mode="bilinear", align_corners=False)`` in one pass.
    lat_affine = (scale, shift) from ``group_norm_affine``: the lateral operand is read as lateral * scale + shift (its
    GroupNorm applied on the fly)."""
    N, C, H, W = lateral.shape
    if not (_fused_map_ok(lateral) and top.dtype == torch.float32):
        _torch_path("upsample_add", lateral, "needs contiguous fp32 NCHW")
        import torch.nn.functional as F
        if lat_affine is not None:
            lateral = lateral * lat_affine[0].view(N, C, 1, 1) + lat_affine[1].view(N, C, 1, 1)
        return lateral + F.interpolate(top, size=(H, W), mode="bilinear", align_corners=False)
    top = top.contiguous()
    out = torch.empty_like(lateral)
    scale, shift = (None, None) if lat_affine is None else (native.dev_ptr(lat_affine[0], "scale"),
                                                            native.dev_ptr(lat_affine[1], "shift"))
    with torch.cuda.device(lateral.device):
        rc = native.lib().dvis_upsample_add(native.dev_ptr(lateral, "lateral"), scale, shift, native.dev_ptr(top, "top"),
                                            native.dev_ptr(out, "out"), N * C, H, W, top.shape[-2], top.shape[-1],
                                            native.stream_ptr(lateral.device))
    native.check(rc, "dvis_upsample_add")
    return out


def _dwconv3x3_tokens_check(op, x, level_shapes, weight):
    B, N, C = x.shape
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and weight.dtype == torch.float32 and C % 4 == 0
            and sum(h * w for h, w in level_shapes) == N and weight.shape == (C, 1, 3, 3)):
        raise RuntimeError(f"{op}: needs a contiguous float32 GPU (B, N, C) tensor, C % 4 == 0, levels summing to N "
                           f"(x {tuple(x.shape)}, levels {list(level_shapes)})")


def _dwconv3x3_tokens_kernel(x, level_shapes, weight, bias, gelu):
    B, N, C = x.shape
    _dwconv3x3_tokens_check("dwconv3x3_tokens", x, level_shapes, weight)
    out = torch.empty_like(x)
    wt = weight.detach().reshape(C, 9).contiguous()
    bptr = None if bias is None else native.dev_ptr(bias.detach().contiguous(), "bias")
    off = 0
    with torch.cuda.device(x.device):
        for h, w in level_shapes:
            rc = native.lib().dvis_dwconv3x3_tokens(ctypes.c_void_p(x.data_ptr() + 4 * off * C), ctypes.c_void_p(out.data_ptr() + 4 * off * C),
                                                    N * C, B, h, w, C, native.dev_ptr(wt, "weight"), bptr, int(gelu),
                                                    native.stream_ptr(x.device))
            native.check(rc, "dvis_dwconv3x3_tokens")
            off += h * w
    return out


def dwconv3x3_tokens_backward(x, level_shapes, weight, bias, grad_out, gelu=False):
    """Backward of ``dwconv3x3_tokens`` (csrc/dwconv_tokens_backward.hip, one call per level): x the forward's input, grad_out
    laid out like it -> (grad_x (B, N, C), grad_weight (C, 1, 3, 3), grad_bias (C) or None without a bias).  Exact fp32 without
    atomics; the levels' weight / bias gradients are added in level order, so every call gives the same bits."""
    B, N, C = x.shape
    _dwconv3x3_tokens_check("dwconv3x3_tokens_backward", x, level_shapes, weight)
    if not (grad_out.is_cuda and grad_out.dtype == torch.float32 and grad_out.shape == x.shape):
        raise RuntimeError(f"dwconv3x3_tokens_backward: grad_out must be a float32 GPU tensor shaped like x (got {tuple(grad_out.shape)})")
    grad_out = grad_out.contiguous()
    dev, lib = x.device, native.lib()
    wt = weight.detach().reshape(C, 9).contiguous()
    bptr = None if bias is None else native.dev_ptr(bias.detach().contiguous(), "bias")
    grad_x = torch.empty_like(x)
    # per level: grad_weight (C, 9) then grad_bias (C)
    part = torch.empty((len(level_shapes), 10 * C), dtype=torch.float32, device=dev)
    nbytes = max(lib.dvis_dwconv3x3_tokens_backward_ws_bytes(B, h, w, C) for h, w in level_shapes)
    ws = torch.empty((max(nbytes, 16) // 4,), dtype=torch.float32, device=dev)      # shared by the levels (same stream: in order)
    off = 0
    with torch.cuda.device(dev):
        for i, (h, w) in enumerate(level_shapes):
            base = 4 * off * C
            rc = lib.dvis_dwconv3x3_tokens_backward(
                ctypes.c_void_p(x.data_ptr() + base), ctypes.c_void_p(grad_out.data_ptr() + base), native.dev_ptr(wt, "weight"), bptr,
                int(gelu), N * C, B, h, w, C, ctypes.c_void_p(grad_x.data_ptr() + base), ctypes.c_void_p(part[i].data_ptr()),
                ctypes.c_void_p(part[i].data_ptr() + 4 * 9 * C) if bias is not None else None, native.dev_ptr(ws, "workspace"),
                native.stream_ptr(dev))
            native.check(rc, "dvis_dwconv3x3_tokens_backward")
            off += h * w
    total = part[0].clone()
    for i in range(1, len(level_shapes)):
        total += part[i]
    return grad_x, total[:9 * C].reshape(C, 1, 3, 3), (total[9 * C:] if bias is not None else None)


class DWConvTokensFunction(Function):
    """``dwconv3x3_tokens`` under autograd: the forward kernel; nothing but x, weight and bias is saved, the backward
    recomputes the pre-activation (csrc/dwconv_tokens_backward.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, level_shapes, gelu):
        ctx.save_for_backward(x, weight, bias)
        ctx.level_shapes, ctx.gelu = [tuple(s) for s in level_shapes], bool(gelu)
        return _dwconv3x3_tokens_kernel(x, level_shapes, weight, bias, gelu)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, weight, bias = ctx.saved_tensors
        gx, gw, gb = dwconv3x3_tokens_backward(x, ctx.level_shapes, weight, bias, grad_out, ctx.gelu)
        need = ctx.needs_input_grad
        return gx if need[0] else None, gw if need[1] else None, gb if bias is not None and need[2] else None, None, None


def dwconv3x3_tokens(x, level_shapes, weight, bias, gelu=False):
    """Depthwise 3x3 convolution (+ bias, + exact GELU) of every pyramid level of a token tensor x (B, N, C) whose levels
    `level_shapes` = [(h, w), ...] are stored one after the other along N (dvis_dwconv3x3_tokens, one launch per level).
    weight (C, 1, 3, 3).  fp32 contiguous GPU tensors.  Differentiable: with grad enabled and an input that requires grad the
    call goes through DWConvTokensFunction."""
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        _dwconv3x3_tokens_check("dwconv3x3_tokens", x, level_shapes, weight)
        return DWConvTokensFunction.apply(x, weight, bias, level_shapes, gelu)
    return _dwconv3x3_tokens_kernel(x, level_shapes, weight, bias, gelu)


def adapter_res2(g, c1, x1_tokens, scale, shift, h8, w8):
    """The ViT-Adapter's stride-4 output in one pass (dvis_adapter_res2, include/dvis_hip.h):
    out[b, co, 2y+dy, 2x+dx] = g[(b, y, x), (dy, dx, co)] + scale[co] * (c1 + up4(x1))[b, co, 2y+dy, 2x+dx] + shift[co].
    g (B*h8*w8, 4C) token-major result of the transposed convolution run as a GEMM, c1 (B, C, 2 h8, 2 w8) contiguous NCHW,
    x1_tokens (B, h8/2 * w8/2, C) or None.  fp32 GPU tensors only (the caller keeps the torch composition for the rest)."""
    B, C = c1.shape[0], c1.shape[1]
    for t, name in ((g, "g"), (c1, "c1"), (scale, "scale"), (shift, "shift")) + (((x1_tokens, "x1"),) if x1_tokens is not None else ()):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError(f"adapter_res2: {name} must be a contiguous float32 GPU tensor")
    if g.shape != (B * h8 * w8, 4 * C) or c1.shape != (B, C, 2 * h8, 2 * w8) or \
            (x1_tokens is not None and x1_tokens.shape != (B, (h8 // 2) * (w8 // 2), C)):
        raise RuntimeError(f"adapter_res2: shapes g {tuple(g.shape)}, c1 {tuple(c1.shape)}, x1 "
                           f"{None if x1_tokens is None else tuple(x1_tokens.shape)} do not match a {h8} x {w8} stride-8 grid")
    out = torch.empty_like(c1)
    with torch.cuda.device(c1.device):
        rc = native.lib().dvis_adapter_res2(native.dev_ptr(g, "g"), native.dev_ptr(c1, "c1"),
                                            None if x1_tokens is None else native.dev_ptr(x1_tokens, "x1"),
                                            native.dev_ptr(scale, "scale"), native.dev_ptr(shift, "shift"), native.dev_ptr(out, "out"),
                                            B, C, h8, w8, native.stream_ptr(c1.device))
    native.check(rc, "dvis_adapter_res2")
    return out


# Library GEMMs or the own deterministic kernel (dvis_gemm_nt)?  The tracker / refiner ALWAYS take the own kernel
# (own=True at their call sites: their stream must never carry a library stream-K kernel, csrc/gemm.hip); everything
# else follows this switch.  DVIS_DETERMINISTIC=1: every GEMM of the pipeline that goes through this module is the own
# kernel -> two runs of a clip give bit-identical tensors (the library's split / stream-K kernels do not promise that).
OWN_GEMM_DEFAULT = os.environ.get("DVIS_DETERMINISTIC", "1") != "0"


class gemm_sizes_as:
    """Inside this context dvis_gemm_nt picks its tile configuration as if the problem had `rows` rows (and `batch` batch
    entries), whatever the actual operand has.  A row's result depends on (N, K, configuration) only, so the tracker gets
    the SAME bits for a clip whether its recurrence runs alone (Q rows per GEMM) or stacked with another clip's (2Q rows)."""
    _tls = threading.local()      # per thread: stream()'s phase-B worker thread must not re-size the main thread's GEMMs

    def __init__(self, rows=None, batch=None):
        self.rows, self.batch = rows, batch

    @staticmethod
    def current():
        return getattr(gemm_sizes_as._tls, "pin", (None, None))

    def __enter__(self):
        self.prev = gemm_sizes_as.current()
        gemm_sizes_as._tls.pin = (self.rows, self.batch)

    def __exit__(self, *exc):
        gemm_sizes_as._tls.pin = self.prev


def _gemm_config(M, N, K, batch, config):
    rows, b = gemm_sizes_as.current()
    if config >= 0 or (rows is None and b is None):
        return config
    return native.lib().dvis_gemm_pick_config(rows or M, N, K, b or batch)


def _rows2d(x, K):
    """(..., K) tensor -> (2-D view (M, K) with unit inner stride, row stride in floats); copies only when the leading
    dims do not collapse into one stride."""
    if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= K:
        return x, x.stride(0)
    if not x.is_contiguous():
        x = x.contiguous()
    return x.view(-1, K), K


def gemm_nt(a, w, bias=None, relu=False, res=None, config=-1, out=None):
    """``relu?(a @ w.T + bias + res)`` on the deterministic exact-fp32 MFMA kernel (dvis_gemm_nt).  a (..., K) float32 GPU
    tensor (rows with unit inner stride; a row-sliced 2-D view keeps its row stride), w (N, K) in F.linear's layout (row
    stride >= K allowed), bias (N) or None, res (..., N) or None.  Returns (..., N).  Raises when the kernel cannot serve
    the operands (K or a row stride not a multiple of 4, unaligned base) — there is no silent library fallback here."""
    K = a.shape[-1]
    N = w.shape[0]
    if not (a.is_cuda and a.dtype == torch.float32 and w.dtype == torch.float32 and w.dim() == 2 and w.shape[1] == K
            and w.stride(1) == 1):
        raise RuntimeError("gemm_nt: needs float32 GPU operands a (..., K), w (N, K) with unit inner strides")
    a2, lda = _rows2d(a, K)
    M = a2.shape[0]
    if out is None:
        out = torch.empty((*a.shape[:-1], N), dtype=torch.float32, device=a.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == M * N):
        raise RuntimeError("gemm_nt: out must be a contiguous float32 GPU tensor of M * N elements")
    rp, ldres = None, 0
    if res is not None:
        if res.numel() != out.numel() or res.shape[-1] != N or res.dtype != torch.float32 or not res.is_cuda:
            raise RuntimeError("gemm_nt: res must be a float32 GPU tensor of the output's shape")
        r2, ldres = _rows2d(res, N)
        rp = ctypes.c_void_p(r2.data_ptr())
    bp = None
    if bias is not None:
        if bias.dtype != torch.float32 or bias.numel() != N or not bias.is_contiguous():
            raise RuntimeError("gemm_nt: bias must be a contiguous float32 (N,) tensor")
        bp = ctypes.c_void_p(bias.data_ptr())
    with torch.cuda.device(a.device):
        rc = native.lib().dvis_gemm_nt(ctypes.c_void_p(a2.data_ptr()), lda, 0, ctypes.c_void_p(w.data_ptr()), w.stride(0), 0,
                                       bp, rp, ldres, 0, ctypes.c_void_p(out.data_ptr()), N, 0, M, N, K, 1,
                                       1 if relu else 0, _gemm_config(M, N, K, 1, config), native.stream_ptr(a.device))
    native.check(rc, "dvis_gemm_nt")
    return out


def gemm_nt_stacked(a, w, bias=None, config=-1):
    """`L` projections of one activation matrix as ONE launch: a (M, L * K) holds L operands side by side (operand l =
    columns [l K, (l + 1) K)), w (L, N, K) / bias (L, N) the L layers' ``nn.Linear`` parameters -> (L, M, N) with
    out[l] = a[:, l K:(l + 1) K] @ w[l].T + bias[l] (dvis_gemm_nt_bb: a batched GEMM with a bias per batch entry)."""
    L, N, K = w.shape
    if not (a.is_cuda and a.dtype == torch.float32 and w.dtype == torch.float32 and a.dim() == 2 and a.stride(1) == 1
            and a.shape[1] == L * K and w.is_contiguous()):
        raise RuntimeError("gemm_nt_stacked: needs float32 GPU operands a (M, L * K) with unit inner stride, contiguous w (L, N, K)")
    if bias is not None and not (bias.dtype == torch.float32 and bias.shape == (L, N) and bias.is_contiguous()):
        raise RuntimeError("gemm_nt_stacked: bias must be a contiguous float32 (L, N) tensor")
    M = a.shape[0]
    out = torch.empty((L, M, N), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = native.lib().dvis_gemm_nt_bb(ctypes.c_void_p(a.data_ptr()), a.stride(0), K, ctypes.c_void_p(w.data_ptr()), K, N * K,
                                          None if bias is None else ctypes.c_void_p(bias.data_ptr()), N, None, 0, 0,
                                          ctypes.c_void_p(out.data_ptr()), N, M * N, M, N, K, L, 0,
                                          _gemm_config(M, N, K, L, config), native.stream_ptr(a.device))
    native.check(rc, "dvis_gemm_nt_bb")
    return out


def gemm_ln_ok(a, w, norms=True):
    """Can dvis_gemm_ln serve ``a (..., K) @ w (N, K).T``?  (fp32 GPU inference tensors, K % 16 == 0, K <= 512 — 2048 for a
    call without norms —, N % 4 == 0)"""
    return (a.is_cuda and a.dtype == torch.float32 and w.dtype == torch.float32 and not torch.is_grad_enabled()
            and w.dim() == 2 and w.stride(1) == 1 and w.stride(0) % 4 == 0
            and bool(native.lib().dvis_gemm_ln_supported(max(1, a.numel() // a.shape[-1]), w.shape[0], a.shape[-1],
                                                         1 if norms else 0)))


def gemm_ln(a, w, bias=None, norm1=None, add=None, norm2=None, relu=False, res=None, a_out=None, out=None, config=-1):
    """``x = norm2(norm1(a) + add)``; returns ``(relu?(x @ w.T + bias + res), x)`` — the LayerNorm seam of a post-norm
    transformer block folded into the prologue of the projection that consumes it (csrc/gemm_ln.hip).  Without norms it
    is the latency form of ``gemm_nt`` for launch-bound chains (every operand requested up front, K <= 2048; x is None).  a (..., K) float32
    GPU rows (the producer's RAW residual sum), norm1 / norm2 ``nn.LayerNorm`` modules or None, add (..., K) or None,
    w (N, K), res (..., N) or None.  a_out / out: optional preallocated destinations ((..., K) / (..., N) row views).
    Raises when the kernel cannot serve the operands — no fallback."""
    K = a.shape[-1]
    N = w.shape[0]
    if (add is None) != (norm2 is None):
        raise RuntimeError("gemm_ln: the forms are norm1, add + norm2, norm1 + add + norm2 or none")
    if not gemm_ln_ok(a, w, norm1 is not None or norm2 is not None) or w.shape[1] != K:
        raise RuntimeError(f"gemm_ln: operands not served (a {tuple(a.shape)} {a.dtype}, w {tuple(w.shape)}; needs fp32 GPU, "
                           "K % 16 == 0, K <= 512, N % 4 == 0, no autograd)")
    a2, lda = _rows2d(a, K)
    M = a2.shape[0]
    lead = a.shape[:-1]

    def rows(t, width, name):
        if t is None:
            return None, 0
        if t.dtype != torch.float32 or not t.is_cuda or t.shape[-1] != width or t.numel() != M * width:
            raise RuntimeError(f"gemm_ln: {name} must be a float32 GPU tensor of {M} rows x {width}")
        t2, ld = _rows2d(t, width)
        return t2, ld
    add2, ldadd = rows(add, K, "add")
    res2, ldres = rows(res, N, "res")
    if a_out is None and (norm1 is not None or norm2 is not None):
        a_out = torch.empty((*lead, K), dtype=torch.float32, device=a.device)
    if out is None:
        out = torch.empty((*lead, N), dtype=torch.float32, device=a.device)
    ao2, ldao = rows(a_out, K, "a_out")
    o2, ldc = rows(out, N, "out")
    if (ao2 is not None and ao2.data_ptr() != a_out.data_ptr()) or o2.data_ptr() != out.data_ptr():
        raise RuntimeError("gemm_ln: a_out / out must be row views (unit inner stride, one row stride)")

    def affine(n):
        if n is None:
            return None, None, 0.0
        if n.weight is None or n.weight.numel() != K or n.weight.dtype != torch.float32:
            raise RuntimeError("gemm_ln: needs an affine float32 LayerNorm over the K columns")
        return ctypes.c_void_p(n.weight.data_ptr()), ctypes.c_void_p(n.bias.data_ptr()), float(n.eps)
    g1, b1, e1 = affine(norm1)
    g2, b2, e2 = affine(norm2)
    rows_pin, _ = gemm_sizes_as.current()
    cfg = config if config >= 0 or rows_pin is None else native.lib().dvis_gemm_ln_pick_config(rows_pin, N, K)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(a.device):
        rc = native.lib().dvis_gemm_ln(ptr(a2), lda, ptr(add2), ldadd, g1, b1, e1, g2, b2, e2, ptr(ao2), ldao,
                                       ctypes.c_void_p(w.data_ptr()), w.stride(0), None if bias is None else ptr(bias.detach()),
                                       ptr(res2), ldres, ptr(o2), ldc, M, N, K, 1 if relu else 0, cfg,
                                       native.stream_ptr(a.device))
    native.check(rc, "dvis_gemm_ln")
    return out, a_out


def bmm_nt(a, b, config=-1):
    """Batched ``a @ b.transpose(1, 2)`` on dvis_gemm_nt: a (B, M, K), b (B, N, K) contiguous float32 GPU -> (B, M, N)."""
    B, M, K = a.shape
    N = b.shape[1]
    if not (a.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and b.shape == (B, N, K)):
        raise RuntimeError("bmm_nt: needs float32 GPU operands a (B, M, K), b (B, N, K)")
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty((B, M, N), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = native.lib().dvis_gemm_nt(ctypes.c_void_p(a.data_ptr()), K, M * K, ctypes.c_void_p(b.data_ptr()), K, N * K, None,
                                       None, 0, 0, ctypes.c_void_p(out.data_ptr()), N, M * N, M, N, K, B, 0,
                                       _gemm_config(M, N, K, B, config), native.stream_ptr(a.device))
    native.check(rc, "dvis_gemm_nt")
    return out


def _own_gemm_ok(x, weight):
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and not torch.is_grad_enabled()
            and x.shape[-1] % 4 == 0 and weight.stride(-1) == 1 and weight.stride(0) % 4 == 0
            and weight.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0)


def linear(x, weight, bias=None, relu=False, own=None, tall=False, act=None, residual=None):
    """``F.linear`` (+ optional ReLU) on fp32 GPU inference tensors WITHOUT a library GEMM, in a form whose result for a row does
    not depend on how many rows share the call (the segmenter folds frames into the batch; a frame must get the same bits alone,
    in a 30-frame clip or in a rank's shard of it):
      tall=True   a projection over every pixel / token of every frame: the split-f16 matrix-core kernel (csrc/gemm_x3.hip)
                  where it is on and serves the shape, else the own exact GEMM from its ONE-WAVE family (K unsplit);
      default     the decoder's small GEMMs (rows = frames x queries): the own exact GEMM from the K-split family of its K
                  (4 waves, 8 from K = 1024 on) — dvis_gemm_pick_config_nw: every tile size of a family sums in the same order;
      own=True    the tracker / refiner call sites: the own GEMM with the size-driven configuration (their batch is pinned
                  with gemm_sizes_as), raising on operands it cannot serve.
    DVIS_DETERMINISTIC=0 hands the non-forced calls back to the library (hipBLASLt: faster on some tall exact shapes, bits that
    change with the row count).  CPU tensors, autograd, autocast / half precision always take torch ops."""
    forced = own is True
    gpu_inf = x.is_cuda and not torch.is_grad_enabled() and not torch.is_autocast_enabled()
    if tall and not forced and gpu_inf and x3_on() and weight.dim() == 2 and weight._base is None \
            and x3_tile_ok(x, weight.shape[0], weight.shape[1]):
        return x3_tile_linear(x, weight, bias, act="relu" if relu and act is None else act, residual=residual)
    if tall and not forced and gpu_inf and x3_on() and weight.dim() == 2 and weight._base is None \
            and x3_ok(x, weight.shape[0], weight.shape[1]):
        # Weights that are views (slices made per call) would be re-packed per call: they stay on the exact kernels below.
        if (act is not None or residual is not None) and weight.shape[0] % 256 == 0:
            return x3_linear(x, weight, bias, relu=relu, act=act, residual=residual)
        if act is None and residual is None:
            return x3_linear(x, weight, bias, relu=relu)
    if act is not None or residual is not None:
        # act ("gelu": the exact erf form of nn.GELU()) / residual (added after it): fused into the split-f16 kernel's epilogue
        # above; everywhere else the same composition in separate passes
        y = linear(x, weight, bias, relu=relu or act == "relu", own=own, tall=tall)
        if act == "gelu":
            y = torch.nn.functional.gelu(y)
        if residual is None:
            return y
        # in place only where that cannot change the result's dtype: under torch.autocast y is fp16 / bf16 and the reference's
        # `x = x + ls(attn(norm(x)))` promotes to the residual stream's fp32
        if not torch.is_grad_enabled() and y.dtype == residual.dtype and not torch.is_autocast_enabled() \
                and not torch.is_autocast_enabled("cpu"):
            return y.add_(residual)
        return residual + y
    own = OWN_GEMM_DEFAULT if own is None else own
    if own and x.is_cuda and not torch.is_grad_enabled() and (forced or not torch.is_autocast_enabled()):
        # (under torch.autocast — how the reference evaluates, train_net_video.py:259 — the projections are torch's half-precision
        # GEMMs: their fp16 / bf16 outputs feed the half-precision fused MSDeformAttn kernel)
        if not forced and not _own_gemm_ok(x, weight) and x.dtype == torch.float32 and weight.dtype == torch.float32 \
                and x.shape[-1] % 4 == 0:
            # a view whose rows are not 16-byte aligned / unit-strided (a slice of the last dim, a transposed weight): one copy
            # makes it servable — cheaper than letting the call fall to the library with other bits per batch size
            if x.stride(-1) != 1 or x.data_ptr() % 16:
                x = x.contiguous()
            if weight.stride(-1) != 1 or weight.stride(0) % 4 or weight.data_ptr() % 16:
                weight = weight.contiguous()
        if _own_gemm_ok(x, weight):
            cfg = -1
            if not forced:
                K = x.shape[-1]
                cfg = native.lib().dvis_gemm_pick_config_nw(max(1, x.numel() // K), weight.shape[0], K, 1,
                                                            1 if tall else (8 if K >= 1024 else 4))
            return gemm_nt(x, weight.detach(), None if bias is None else bias.detach().contiguous(), relu=relu, config=cfg)
        if forced:
            # tracker / refiner call sites: their stream must NEVER carry a library (stream-K) GEMM and every rank must
            # compute the same bits — a refused operand is an error whatever DVIS_STRICT says (as in gemm_nt itself)
            raise RuntimeError(f"linear(own=True): the own GEMM cannot serve these operands (needs fp32, K % 4 == 0, 16-byte "
                               f"aligned operands, weight row stride % 4 == 0; x {tuple(x.shape)} {x.dtype}, weight "
                               f"{tuple(weight.shape)} {weight.dtype} stride {tuple(weight.stride())})")
        # (K % 4 != 0 or mixed dtypes: no layer of the reference's configurations; the library GEMM below serves them)
    if relu and bias is not None and x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled():
        K = x.shape[-1]
        y = torch._addmm_activation(bias, x.reshape(-1, K), weight.t(), use_gelu=False)
        return y.view(*x.shape[:-1], weight.shape[0])
    y = torch.nn.functional.linear(x, weight, bias)
    return torch.relu(y) if relu else y


def linear_relu(x, lin, own=None, tall=False):
    """relu(lin(x)) for an ``nn.Linear``."""
    return linear(x, lin.weight, lin.bias, relu=True, own=own, tall=tall)


# ---- the encoder's tall GEMMs on the F16 matrix cores (csrc/gemm_x3.hip): fp32 operands as two f16 terms, three products
# per pair, fp32 accumulation -> the error of an fp32 GEMM at 3/16 of its matrix-core time.
X3 = os.environ.get("DVIS_X3", "1") != "0"
# Stages of phase A whose layers stay on the exact-fp32 kernels although X3 is on: a comma-separated subset of
# backbone, pd_proj (the pixel decoder's input projections), mask_path (lateral 1x1 + FPN 3x3 + mask_features 1x1), encoder
# (MSDeformAttn projections + FFN), decoder_kv (the masked-attention decoder's key / value projections).  The callers mark their stage with `x3_stage(name)`.
X3_OFF = frozenset(v for v in os.environ.get("DVIS_X3_OFF", "").split(",") if v)
_x3_tls = threading.local()


class x3_stage:
    """``with x3_stage("encoder"): ...`` — names the stage the enclosed calls belong to (per thread), for X3_OFF."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.prev = getattr(_x3_tls, "stage", None)
        _x3_tls.stage = self.name

    def __exit__(self, *exc):
        _x3_tls.stage = self.prev


def x3_on():
    """Split-f16 matrix-core kernels for the calling stage?  (the master switch X3 / DVIS_X3, minus the stages in X3_OFF, and not
    inside an `x3_disabled()` block)"""
    return X3 and not getattr(_x3_tls, "disabled", 0) and not (X3_OFF and getattr(_x3_tls, "stage", None) in X3_OFF)


class x3_disabled:
    """``with x3_disabled(): ...`` — the enclosed calls (this thread) take the exact-fp32 kernels: the re-run after an X3RangeError."""

    def __enter__(self):
        _x3_tls.disabled = getattr(_x3_tls, "disabled", 0) + 1

    def __exit__(self, *exc):
        _x3_tls.disabled -= 1


class X3RangeError(RuntimeError):
    """An activation left the f16 range of the split-f16 kernels (|x| >= 65520 / 2^xexp: 4095 in the linear / FFN kernels at
    DVIS_X3_XEXP = 4, 16380 in the convolutions at DVIS_X3_CONV_XEXP = 2): the layer's output rows are non-finite."""


# what DVIS_Plus_* do with an X3RangeError on a single GPU: "rerun" the clip on the exact-fp32 kernels with a warning (and keep
# that model on them from then on), or "raise".  Sharded runs always raise: the other ranks already hold the gathered queries.
X3_ON_OVERFLOW = os.environ.get("DVIS_X3_ON_OVERFLOW", "rerun")


class _X3RangeGuard:
    """Host side of the kernels' range guard (include/dvis_hip.h: dvis_x3_set_range_flag / dvis_x3_set_tag).  One sticky int32
    word per device receives the TAG of a launch that produced a non-finite pre-activation value; every packed weight gets a
    tag, so the word names the layer.  `snapshot()` (after phase A of a clip is enqueued) copies the word to pinned memory
    behind the clip's kernels — no synchronisation; `verify()` (before the clip's results are used) waits for that copy."""

    def __init__(self):
        self.words, self.pool, self.tags, self.lock = {}, {}, {}, threading.Lock()
        self.next_tag = 1

    def word(self, device):
        idx = device.index if device.index is not None else torch.cuda.current_device()
        w = self.words.get(idx)
        if w is None:
            with self.lock:
                w = self.words.get(idx)
                if w is None:
                    w = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
                    with torch.cuda.device(idx):
                        native.check(native.lib().dvis_x3_set_range_flag(ctypes.c_void_p(w.data_ptr())), "dvis_x3_set_range_flag")
                    # (pool before words: a lock-free reader that finds the word must find its pinned buffers too)
                    self.pool[idx] = [[torch.zeros(1, dtype=torch.int32).pin_memory() for _ in range(16)], 0]
                    self.words[idx] = w
        return w

    def new_tag(self, weight, kind):
        import weakref
        with self.lock:
            tag = self.next_tag
            self.next_tag += 1
            self.tags[tag] = (kind, weakref.ref(weight), tuple(weight.shape))
        return tag

    def snapshot(self, device):
        if not (X3 and device.type == "cuda"):
            return None
        w = self.word(device)
        idx = w.device.index
        bufs = self.pool[idx]
        host = bufs[0][bufs[1] % len(bufs[0])]
        bufs[1] += 1
        host.copy_(w, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(w.device))
        # (4th entry: the word's value at this point of the stream as a DEVICE tensor — what a sharded run sends through the
        # clip's all-gather so that every rank takes the same decision, clip_shard.all_gather_frames)
        return (host, ev, w, w.clone())

    def describe(self, tag, model=None):
        kind, ref, shape = self.tags.get(tag, ("?", lambda: None, ()))
        wt, name = ref(), None
        if wt is not None and model is not None:
            for n, mod in model.named_modules():
                for pn, prm in list(mod.named_parameters(recurse=False)) + list(mod.named_buffers(recurse=False)):
                    if prm is wt:
                        name = f"{n}.{pn}"
                if name is None and getattr(mod, "is_folded_weight", lambda t: False)(wt):
                    name = f"{n} (FrozenBN folded)"
                if name:
                    break
        return f"{name or 'weight'} {shape} [{kind} kernel]"

    def verify(self, snap, model=None):
        if snap is None:
            return
        host, ev, w = snap[:3]
        ev.synchronize()
        self.raise_if(int(host[0]), w, model)

    def verify_gathered(self, tags, device, model=None):
        """The collective form: `tags` = every rank's guard word as gathered with the clip's queries (float tensor).  Same
        data on every rank -> every rank raises (or none does)."""
        if tags is None:
            return
        self.raise_if(int(tags.max().item()), self.word(device), model)

    def raise_if(self, tag, w, model=None):
        if tag:
            w.zero_()
            raise X3RangeError(
                f"split-f16 range exceeded in {self.describe(tag, model)}: an input activation (or the FFN's hidden activation) "
                f"reached |x| >= 65520 / 2^xexp (xexp = {X3_XEXP} in the linear / FFN kernels, {X3_CONV_XEXP} in the convolutions) and "
                "the layer's outputs are non-finite.  Exact-fp32 kernels: DVIS_X3=0 (everything) or DVIS_X3_OFF=<stage,...> "
                "(backbone, pd_proj, mask_path, encoder, decoder_kv); more range at the cost of small-value precision: "
                "DVIS_X3_XEXP / DVIS_X3_CONV_XEXP.")

    def check_now(self, device, model=None):
        """Synchronous form (tests, one-off calls): reads the word after a device synchronisation."""
        self.verify(self.snapshot(device), model)


X3_GUARD = _X3RangeGuard()


def x3_range_snapshot(device):
    return X3_GUARD.snapshot(device)


def x3_range_verify(snap, model=None):
    X3_GUARD.verify(snap, model)


X3_XEXP = int(os.environ.get("DVIS_X3_XEXP", "4"))      # activations are scaled by 2^4 before the split (|x| < 4095 = 65520 / 2^4)
# the convolutions see ReLU'd feature maps without a normalisation in front: more range (|x| < 16380 = 65520 / 2^2), an absolute floor of
# 2^-27 = 7.5e-9 per element below |x| = 0.03
X3_CONV_XEXP = int(os.environ.get("DVIS_X3_CONV_XEXP", "2"))
# conv1x1_bias_act: from this many input channels on a 1x1 layer goes to the split-f16 kernel first — also the memory-bound
# ones csrc/conv1x1.hip (weights resident in LDS, exact fp32) was written for: 64 -> 256 + shortcut at 184 x 320 runs at 5.0
# TB/s there against 4.3, 256 -> 128 in 0.62 ms against 1.13 (tools/x3_time.py conv)
X3_CONV1X1_MIN_CI = int(os.environ.get("DVIS_X3_CONV1X1_MIN_CI", "64"))


def _x3_exp(w):
    """e with max|w| * 2^e in [2^13, 2^14): the weight fills the f16 range, its low term stays a normal number."""
    m = float(w.detach().abs().max())
    return 0 if m == 0.0 or m != m else 14 - math.frexp(m)[1]


def _x3_wexp(w):
    """_x3_exp(w) within the +-60 the pack kernels take: 2^wexp travels as a float, and so does the epilogues' 2^-(xexp + wexp).
    Only a matrix whose largest element is below 2^-46 (or above 2^74) is affected — one with max|w| below 2^-85 packs as zero."""
    return max(-60, min(60, _x3_exp(w)))


def _x3_cache(key_obj, sources, make, kind="linear"):
    """The split-f16 pack `make()` of `sources`, one per (key_obj, kind) in derived.TABLE; every pack has its own range-guard tag."""
    ent = derived.TABLE.entry(key_obj, kind, sources, make, note=lambda: X3_GUARD.new_tag(key_obj, kind))
    # the launch that follows carries this weight's tag (range guard; per host thread) — and the device's guard word exists
    X3_GUARD.word(key_obj.device)
    native.lib().dvis_x3_set_tag(ent.note)
    return ent.value


def _x3_packed(w, nbytes, pack, name):
    """(packed uint8 buffer of `nbytes`, wexp) of the contiguous weight `w` through `pack(wexp, buffer pointer, stream)`."""
    e = _x3_wexp(w)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    with torch.cuda.device(w.device):
        native.check(pack(e, ctypes.c_void_p(buf.data_ptr()), native.stream_ptr(w.device)), name)
    return buf, e


def _x3_pack_conv1x1(w2):
    """(packed buffer, wexp) of a contiguous (Co, Ci) matrix for csrc/conv1x1_x3.hip."""
    Co, Ci = w2.shape
    return _x3_packed(w2, native.lib().dvis_conv1x1_x3_packed_bytes(Ci, Co), lambda e, buf, st: native.lib().dvis_conv1x1_x3_pack(
        native.dev_ptr(w2, "weight"), Co, Ci, e, buf, st), "dvis_conv1x1_x3_pack")


def _x3_pack_conv3x3(w4):
    """The same of a contiguous (Co, Ci, 3, 3) weight (nine taps)."""
    Co, Ci = w4.shape[:2]
    return _x3_packed(w4, native.lib().dvis_conv3x3_x3_packed_bytes(Ci, Co), lambda e, buf, st: native.lib().dvis_conv3x3_x3_pack(
        native.dev_ptr(w4, "weight"), Co, Ci, e, buf, st), "dvis_conv3x3_x3_pack")


def x3_pack(weight):
    """(packed uint8 buffer, wexp) of an (N, K) float32 GPU weight, made once per weight version."""
    def make():
        w = weight.detach()
        if w.stride(1) != 1:
            w = w.contiguous()
        N, K = w.shape
        nbytes = native.lib().dvis_x3_packed_bytes(N, K)
        if nbytes <= 0:
            raise RuntimeError(f"x3_pack: weight {tuple(w.shape)} is not served (K % 32 == 0)")
        return _x3_packed(w, nbytes, lambda e, buf, st: native.lib().dvis_x3_pack(
            ctypes.c_void_p(w.data_ptr()), w.stride(0), N, K, e, buf, st), "dvis_x3_pack")
    return _x3_cache(weight, [weight], make)


# The large-K tall GEMMs (ViT blocks: K = 1024 .. 4096, N a multiple of 256) take the TILED split-f16 kernel (csrc/gemm_x3_tile.hip:
# both operands through LDS, one split of the rows per 256 output features); the encoder's K = 256 layers keep the streaming
# kernels with their fused LayerNorm / position forms.  DVIS_X3_TILE_MIN_K (development): K from which the tiled kernel is used.
X3_TILE_MIN_K = int(os.environ.get("DVIS_X3_TILE_MIN_K", "512"))


def x3_tile_ok(x, N, K):
    return (x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and x.shape[-1] == K and K >= X3_TILE_MIN_K
            and bool(native.lib().dvis_x3_tile_supported(N, K)))


def x3_tile_pack(weight, order=0):
    """(packed buffer, wexp) of an (N, K) float32 GPU weight in the tiled kernel's LDS image, made once per weight version.
    order: the k-slot order of the row image the weight meets (RowImage.order; 0 for fp32 rows)."""
    def make():
        w = weight.detach()
        if w.stride(1) != 1:
            w = w.contiguous()
        N, K = w.shape
        nbytes = native.lib().dvis_x3_tile_packed_bytes(N, K)
        if nbytes <= 0:
            raise RuntimeError(f"x3_tile_pack: weight {tuple(w.shape)} is not served (N % 256 == 0, K % 32 == 0)")
        return _x3_packed(w, nbytes, lambda e, buf, st: native.lib().dvis_x3_tile_pack(
            ctypes.c_void_p(w.data_ptr()), w.stride(0), N, K, e, order, buf, st), "dvis_x3_tile_pack")
    return _x3_cache(weight, [weight], make, kind="tile" if order == 0 else f"tile order {order}")


# Row images (include/dvis_hip.h, "ROW IMAGES"; csrc/gemm_x3_tile.hip): the tiled GEMM's row operand pre-split by its producer.
# DVIS_X3_ROW_IMAGES=0 (development): the ViT blocks keep fp32 activations between their layers.
X3_ROW_IMAGES = os.environ.get("DVIS_X3_ROW_IMAGES", "1") != "0"


class RowImage:
    """fp32 rows (..., K) as the row operand image of dvis_x3_tile_linear_image: `data` (uint8, dvis_x3_rows_image_bytes), `shape` of
    the tensor it stands for, `exp` (values x 2^exp before the split), `order` (k-slot order: the weights are packed to match)."""

    def __init__(self, data, shape, exp, order):
        self.data, self.shape, self.exp, self.order = data, tuple(shape), exp, order

    @property
    def device(self):
        return self.data.device

    @property
    def rows(self):
        n = 1
        for d in self.shape[:-1]:
            n *= d
        return n


def _rows_image_buffer(M, K, device):
    nbytes = native.lib().dvis_x3_rows_image_bytes(M, K)
    if nbytes < 0:
        raise RuntimeError(f"row image: K % 32 == 0 is required (K {K})")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def x3_rows_image(x, xexp=None):
    """fp32 GPU rows (..., K) -> RowImage (order 0): the stand-alone producer."""
    K = x.shape[-1]
    x2, ldx = _x3_rows(x, "x")
    e = X3_XEXP if xexp is None else xexp
    buf = _rows_image_buffer(x2.shape[0], K, x.device)
    with torch.cuda.device(x.device):
        native.check(native.lib().dvis_x3_rows_image(ctypes.c_void_p(x2.data_ptr()), ldx, x2.shape[0], K, e, ctypes.c_void_p(buf.data_ptr()),
                                                     native.stream_ptr(x.device)), "dvis_x3_rows_image")
    return RowImage(buf, x.shape, e, 0)


def layer_norm_rows_image_ok(x, norm):
    C = x.shape[-1]
    return (X3_ROW_IMAGES and x3_on() and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0
            and C % 32 == 0 and C <= 1024 and norm.weight is not None and norm.bias is not None and not torch.is_grad_enabled()
            and not torch.is_autocast_enabled())


def layer_norm_rows_image(x, norm, xexp=None):
    """``norm(x)`` (nn.LayerNorm over the last dim) written as the RowImage (order 0) of the GEMM that reads it — the value every
    element holds is add_layer_norm's, split into its two f16 terms."""
    C = x.shape[-1]
    M = x.numel() // C
    e = X3_XEXP if xexp is None else xexp
    buf = _rows_image_buffer(M, C, x.device)
    with torch.cuda.device(x.device):
        native.check(native.lib().dvis_layernorm_rows_image(
            ctypes.c_void_p(x.data_ptr()), native.dev_ptr(norm.weight, "gamma"), native.dev_ptr(norm.bias, "beta"), M, C, float(norm.eps), e,
            ctypes.c_void_p(buf.data_ptr()), native.stream_ptr(x.device)), "dvis_layernorm_rows_image")
    return RowImage(buf, x.shape, e, 0)


def x3_tile_linear(x, weight, bias, act=None, residual=None, xexp=None):
    """``act(x @ weight.T + bias) + residual`` (act: None | "relu" | "gelu") through dvis_x3_tile_linear, or for x a RowImage
    through dvis_x3_tile_linear_image: act None / "relu" -> fp32 rows (+ residual); act "gelu" -> the next GEMM's RowImage."""
    N, K = weight.shape
    image_in = isinstance(x, RowImage)
    image_out = image_in and act == "gelu"
    # the row operand: (image, rows) or (fp32 rows, row stride, rows); its exponent; the k order its weights are packed in
    if image_in:
        if x.shape[-1] != K:
            raise RuntimeError(f"x3_tile_linear: image of {x.shape} rows against a weight of {tuple(weight.shape)}")
        entry = "dvis_x3_tile_linear_image"
        xargs, x_exp, order = (ctypes.c_void_p(x.data.data_ptr()), x.rows), x.exp, x.order
    else:
        x2, ldx = _x3_rows(x, "x")
        entry = "dvis_x3_tile_linear"
        xargs, x_exp, order = (ctypes.c_void_p(x2.data_ptr()), ldx, x2.shape[0]), X3_XEXP if xexp is None else xexp, 0
    buf, wexp = x3_tile_pack(weight, order)
    # the output: (residual, its stride, fp32 rows, their stride), and for the image entry (row image, its exponent) behind them
    no_rows, no_image = (None, 0, None, 0), (None, 0)
    if image_out:
        if residual is not None:
            raise RuntimeError("x3_tile_linear: the GELU form of a row image writes a row image (no residual)")
        out = _rows_image_buffer(x.rows, N, x.device)
        oargs = (*no_rows, ctypes.c_void_p(out.data_ptr()), X3_XEXP)
    else:
        out = torch.empty((*x.shape[:-1], N), dtype=torch.float32, device=x.device)
        rows_out = (*_x3_residual("x3_tile_linear", residual, out), ctypes.c_void_p(out.data_ptr()), N)
        oargs = (*rows_out, *no_image) if image_in else rows_out
    with torch.cuda.device(x.device):
        native.check(getattr(native.lib(), entry)(
            *xargs, K, ctypes.c_void_p(buf.data_ptr()), N, x_exp, wexp, None if bias is None else native.dev_ptr(bias.detach(), "bias"),
            {None: 0, "relu": 1, "gelu": 2}[act], *oargs, native.stream_ptr(x.device)), entry)
    return RowImage(out, (*x.shape[:-1], N), X3_XEXP, 1) if image_out else out


X3_QKV_FUSED = os.environ.get("DVIS_X3_QKV_FUSED", "1") != "0"


def x3_qkv_attention_ok(x, weight, heads):
    """Can ``self_attention(x @ weight.T + bias)`` take the fused form (dvis_x3_tile_linear_qkv + dvis_attention_x3_packed)?
    x (B, L, C) float32 GPU inference tensor, weight (3C, C), head dim 64, L >= 1024 (the ViT blocks)."""
    if len(x.shape) != 3 or not (X3_QKV_FUSED and weight.dim() == 2 and weight._base is None):
        return False
    if not isinstance(x, RowImage) and not (
            x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and not torch.is_autocast_enabled() and x3_on()
            and x.is_contiguous() and x.data_ptr() % 16 == 0):
        return False
    B, L, C = x.shape
    return (C == heads * 64 and weight.shape == (3 * C, C) and L >= 1024 and C >= X3_TILE_MIN_K
            and bool(native.lib().dvis_x3_tile_supported(3 * C, C)))


def x3_qkv_attention(x, weight, bias, heads, out_image=False):
    """softmax(q k^T / 8) v per head for qkv = x @ weight.T + bias (columns ordered q | k | v, head, dim), x (B, L, C), head dim 64:
    the projection's epilogue writes the split-f16 attention kernel's operand images, the attention kernel reads them — the fp32
    qkv tensor and the pack pass do not exist.  x: fp32 tensor or RowImage.  -> (B, L, C) fp32, or with out_image its RowImage
    (order 2: the out-projection's row operand)."""
    B, L, C = x.shape
    image_in = isinstance(x, RowImage)
    buf, wexp = x3_tile_pack(weight, x.order if image_in else 0)
    lib = native.lib()
    nbytes = lib.dvis_attention_ws_bytes_k(B * heads, L, L, 64, 2)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    qscale = (1.0 / 8.0) * 1.4426950408889634 * 16.0
    bptr = None if bias is None else native.dev_ptr(bias.detach(), "bias")
    with torch.cuda.device(x.device):
        if image_in:
            native.check(lib.dvis_x3_tile_linear_qkv_image(
                ctypes.c_void_p(x.data.data_ptr()), B * L, C, ctypes.c_void_p(buf.data_ptr()), 3 * C, x.exp, wexp, bptr, heads, L, qscale,
                ctypes.c_void_p(ws.data_ptr()), native.stream_ptr(x.device)), "dvis_x3_tile_linear_qkv_image")
        else:
            native.check(lib.dvis_x3_tile_linear_qkv(
                ctypes.c_void_p(x.data_ptr()), C, B * L, C, ctypes.c_void_p(buf.data_ptr()), 3 * C, X3_XEXP, wexp, bptr, heads, L, qscale,
                ctypes.c_void_p(ws.data_ptr()), native.stream_ptr(x.device)), "dvis_x3_tile_linear_qkv")
        if out_image:
            out = _rows_image_buffer(B * L, C, x.device)
            native.check(lib.dvis_attention_x3_packed_image(ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, heads, L, X3_XEXP,
                                                            native.stream_ptr(x.device)), "dvis_attention_x3_packed_image")
            return RowImage(out, (B, L, C), X3_XEXP, 2)
        out = torch.empty((B, L, C), dtype=torch.float32, device=x.device)
        strides = (ctypes.c_int64 * 3)(L * C, 64, C)
        native.check(lib.dvis_attention_x3_packed(ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(out.data_ptr()), strides, B, heads, L,
                                                  native.stream_ptr(x.device)), "dvis_attention_x3_packed")
    return out


def x3_ok(x, N, K, ln=False, add=False):
    """Does csrc/gemm_x3.hip serve ``x (..., K) @ W (N, K).T``?  ln: the output_proj + residual + LayerNorm form; add: the form
    with the in-kernel ``x + xadd`` (dvis_x3_linear_add: K = 256 only)."""
    return (x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and x.shape[-1] == K
            and (not add or K == 256) and bool(native.lib().dvis_x3_linear_supported(N, K, int(ln))))


def _x3_rows(x, name):
    K = x.shape[-1]
    x2, ld = _rows2d(x, K)
    if x2.data_ptr() % 16 or ld % 4:
        raise RuntimeError(f"x3: {name} must be 16-byte aligned with a row stride % 4 == 0")
    return x2, ld


X3_LINEAR_ROWS = os.environ.get("DVIS_X3_LINEAR_ROWS", "1") != "0"


def x3_rows_in_place(x, N):
    """Is ``x`` a (B, S, K) slice of a longer (B, S', K) tensor — unit inner stride, row stride K, a batch stride that is a multiple
    of 4 floats — whose rows dvis_x3_linear_rows / _add_rows read where they lie (N % 256 == 0)?  Otherwise, and with
    DVIS_X3_LINEAR_ROWS=0, ``x3_linear`` compacts such a view first."""
    return (X3_LINEAR_ROWS and x.dim() == 3 and not x.is_contiguous() and x.shape[0] > 0 and x.shape[1] > 0 and N % 256 == 0
            and x.stride(2) == 1 and x.stride(1) == x.shape[2] and x.stride(0) % 4 == 0 and x.stride(0) >= x.shape[1] * x.shape[2]
            and x.data_ptr() % 16 == 0)


def _x3_residual(op, residual, out, rows=_rows2d):
    """(pointer, row stride) of the optional `residual` added to the fp32 GPU rows `out`; (None, 0) without one."""
    if residual is None:
        return None, 0
    if residual.shape != out.shape or residual.dtype != torch.float32 or not residual.is_cuda:
        raise RuntimeError(f"{op}: residual must be a float32 GPU tensor of the output's shape")
    r2, ldr = rows(residual, out.shape[-1])
    return ctypes.c_void_p(r2.data_ptr()), ldr


def x3_linear(x, weight, bias, relu=False, xexp=None, xadd=None, act=None, residual=None):
    """``relu?((x + xadd) @ weight.T + bias)`` through dvis_x3_linear[_add]; with act ("gelu" | "relu" | None) / residual:
    ``act(x @ weight.T + bias) + residual`` through dvis_x3_linear_res (GELU and the residual add inside the GEMM's epilogue).  x (..., K) float32 GPU; weight (N, K); xadd: None or
    a (1, S, 256) / (S, 256) embedding for x of shape (B, S, 256), broadcast over B — added inside the kernel while it builds the
    row's fragments, the sum is never written (K = 256, any N the kernels serve: all passes over N run from one read of the row).
    A (B, S, K) slice of a longer tensor (``x3_rows_in_place``) is read where it lies: dvis_x3_linear_rows / _add_rows."""
    N, K = weight.shape
    in_place = act is None and residual is None and x3_rows_in_place(x, N)
    if in_place:        # x, row stride, rows per batch entry, batch stride, rows
        xargs = (ctypes.c_void_p(x.data_ptr()), K, x.shape[1], x.stride(0), x.shape[0] * x.shape[1])
    else:
        x2, ldx = _x3_rows(x, "x")
        xargs = (ctypes.c_void_p(x2.data_ptr()), ldx, x2.shape[0])
    buf, wexp = x3_pack(weight)
    out = torch.empty((*x.shape[:-1], N), dtype=torch.float32, device=x.device)
    wargs = (K, ctypes.c_void_p(buf.data_ptr()), N, X3_XEXP if xexp is None else xexp, wexp)
    bptr = None if bias is None else native.dev_ptr(bias.detach(), "bias")
    oargs = (ctypes.c_void_p(out.data_ptr()), N, native.stream_ptr(x.device))
    if act is not None or residual is not None:
        if xadd is not None:
            raise RuntimeError("x3_linear: xadd and act / residual are served by different entry points")
        code = {None: int(bool(relu)), "relu": 1, "gelu": 2}[act]
        entry = "dvis_x3_linear_res"
        extra = (bptr, code, *_x3_residual("x3_linear", residual, out, rows=lambda r, _: _x3_rows(r, "residual")))
    elif xadd is not None:
        if x.dim() != 3 or xadd.numel() != x.shape[1] * K or xadd.dtype != torch.float32 or not xadd.is_cuda:
            raise RuntimeError("x3_linear: xadd must be a float32 GPU (S, K) embedding for x of shape (B, S, K)")
        xadd = xadd.contiguous()
        entry = "dvis_x3_linear_add_rows" if in_place else "dvis_x3_linear_add"
        extra = (ctypes.c_void_p(xadd.data_ptr()), x.shape[1], bptr, int(relu))
    else:
        entry = "dvis_x3_linear_rows" if in_place else "dvis_x3_linear"
        extra = (bptr, int(relu))
    with torch.cuda.device(x.device):
        native.check(getattr(native.lib(), entry)(*xargs, *wargs, *extra, *oargs), entry)
    return out


def _x3_pos(pos, x, N):
    if pos is None:
        return None, 0, None
    if x.dim() != 3 or pos.numel() != x.shape[1] * N or pos.dtype != torch.float32 or not pos.is_cuda:
        raise RuntimeError("x3: pos must be a float32 GPU (S, C) embedding for x of shape (N, S, C)")
    return pos.contiguous(), x.shape[1], torch.empty((*x.shape[:-1], N), dtype=torch.float32, device=x.device)


def x3_linear_ln(x, weight, bias, res, norm, pos=None, xexp=None):
    """``norm(res + x @ weight.T + bias)`` (+ second output ``out + pos``) in one kernel (dvis_x3_linear_ln)."""
    N, K = weight.shape
    x2, ldx = _x3_rows(x, "x")
    r2, ldr = _x3_rows(res, "res")
    buf, wexp = x3_pack(weight)
    out = torch.empty((*x.shape[:-1], N), dtype=torch.float32, device=x.device)
    pos, pos_rows, out2 = _x3_pos(pos, x, N)
    with torch.cuda.device(x.device):
        native.check(native.lib().dvis_x3_linear_ln(
            ctypes.c_void_p(x2.data_ptr()), ldx, x2.shape[0], K, ctypes.c_void_p(buf.data_ptr()), N,
            X3_XEXP if xexp is None else xexp, wexp, native.dev_ptr(bias.detach(), "bias"), ctypes.c_void_p(r2.data_ptr()), ldr,
            native.dev_ptr(norm.weight.detach(), "gamma"), native.dev_ptr(norm.bias.detach(), "beta"), float(norm.eps),
            None if pos is None else ctypes.c_void_p(pos.data_ptr()), pos_rows, ctypes.c_void_p(out.data_ptr()),
            None if out2 is None else ctypes.c_void_p(out2.data_ptr()), N, native.stream_ptr(x.device)), "dvis_x3_linear_ln")
    return out if out2 is None else (out, out2)


def x3_ffn_ok(x, lin1, lin2):
    K, H, N = lin1.weight.shape[1], lin1.weight.shape[0], lin2.weight.shape[0]
    return (x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and x.shape[-1] == K
            and lin2.weight.shape[1] == H and lin1.bias is not None and lin2.bias is not None
            and native.lib().dvis_x3_ffn_packed_bytes(K, H, N) > 0)


def x3_ffn_ln(x, lin1, lin2, norm, pos=None, xexp=None, hexp=None):
    """``norm(x + lin2(relu(lin1(x))))`` (+ ``out + pos``) in one kernel (dvis_x3_ffn_ln): the hidden tensor stays on chip."""
    w1, w2 = lin1.weight, lin2.weight
    H, K = w1.shape
    N = w2.shape[0]
    x2, ldx = _x3_rows(x, "x")

    def make():
        a, b = w1.detach().contiguous(), w2.detach().contiguous()
        e1, e2 = _x3_wexp(a), _x3_wexp(b)
        buf = torch.empty(native.lib().dvis_x3_ffn_packed_bytes(K, H, N), dtype=torch.uint8, device=a.device)
        with torch.cuda.device(a.device):
            native.check(native.lib().dvis_x3_ffn_pack(ctypes.c_void_p(a.data_ptr()), K, ctypes.c_void_p(b.data_ptr()), H, K, H,
                                                       N, e1, e2, ctypes.c_void_p(buf.data_ptr()),
                                                       native.stream_ptr(a.device)), "dvis_x3_ffn_pack")
        return buf, e1, e2
    buf, e1, e2 = _x3_cache(w1, [w1, w2], make, kind="ffn")
    out = torch.empty((*x.shape[:-1], N), dtype=torch.float32, device=x.device)
    pos, pos_rows, out2 = _x3_pos(pos, x, N)
    with torch.cuda.device(x.device):
        native.check(native.lib().dvis_x3_ffn_ln(
            ctypes.c_void_p(x2.data_ptr()), ldx, x2.shape[0], K, H, N, ctypes.c_void_p(buf.data_ptr()),
            X3_XEXP if xexp is None else xexp, e1, X3_XEXP if hexp is None else hexp, e2,
            native.dev_ptr(lin1.bias.detach(), "b1"), native.dev_ptr(lin2.bias.detach(), "b2"),
            native.dev_ptr(norm.weight.detach(), "gamma"), native.dev_ptr(norm.bias.detach(), "beta"), float(norm.eps),
            None if pos is None else ctypes.c_void_p(pos.data_ptr()), pos_rows, ctypes.c_void_p(out.data_ptr()),
            None if out2 is None else ctypes.c_void_p(out2.data_ptr()), N, native.stream_ptr(x.device)), "dvis_x3_ffn_ln")
    return out if out2 is None else (out, out2)


def maps_to_tokens(maps, affines=None, pos=None):
    """[(N, C, h_l, w_l)] -> (N, sum h_l*w_l, C): ``torch.cat([m.flatten(2).transpose(1, 2) for m in maps], 1)`` with one
    tiled transpose per level instead of torch's strided copy.  CPU / non-fp32 / non-contiguous inputs use the torch ops.
    affines: per level None or (scale, shift) from ``group_norm_affine`` — the map is read as m * scale + shift.
    pos: optional (1, S, C) / (S, C) token-major embedding: returns (tokens, tokens + pos), both written in the one pass."""
    affines = affines or [None] * len(maps)
    N, C = maps[0].shape[:2]
    if not all(m.is_cuda and m.dtype == torch.float32 and m.is_contiguous() for m in maps) or torch.is_grad_enabled():
        _torch_path("maps_to_tokens", maps[0], "needs contiguous fp32 NCHW maps")
        maps = [m if a is None else m * a[0].view(N, C, 1, 1) + a[1].view(N, C, 1, 1) for m, a in zip(maps, affines)]
        out = torch.cat([m.flatten(2).transpose(1, 2) for m in maps], 1)
        return out if pos is None else (out, out + pos.reshape(1, -1, C))
    S = sum(m.shape[2] * m.shape[3] for m in maps)
    out = torch.empty((N, S, C), dtype=torch.float32, device=maps[0].device)
    out_pos = pp = None
    if pos is not None:
        if pos.numel() != S * C or pos.dtype != torch.float32 or not pos.is_cuda:
            raise RuntimeError("maps_to_tokens: pos must be a float32 GPU (S, C) embedding")
        pos = pos.contiguous()
        out_pos = torch.empty_like(out)
        pp = native.dev_ptr(pos, "pos")
    row0 = 0
    with torch.cuda.device(out.device):
        for m, a in zip(maps, affines):
            HW = m.shape[2] * m.shape[3]
            rc = native.lib().dvis_nchw_to_tokens(
                ctypes.c_void_p(m.data_ptr()), None if a is None else native.dev_ptr(a[0], "scale"),
                None if a is None else native.dev_ptr(a[1], "shift"), pp, ctypes.c_void_p(out.data_ptr()),
                None if out_pos is None else ctypes.c_void_p(out_pos.data_ptr()), N, C, HW, S, row0,
                native.stream_ptr(out.device))
            native.check(rc, "dvis_nchw_to_tokens")
            row0 += HW
    return out if pos is None else (out, out_pos)


def normalize_pad_ok(x, mean):
    return bool(x.is_cuda and x.dim() == 4 and x.dtype in (torch.uint8, torch.float32) and x.is_contiguous()
                and mean.numel() == x.shape[1] and mean.dtype == torch.float32 and not torch.is_grad_enabled())


def normalize_pad(x, mean, std, Hp, Wp):
    """zero-padded ((x - mean[c]) / std[c]) of (N, C, H, W) uint8 / fp32 frames as ONE pass: conversion, normalisation and
    ImageList.from_tensors' padding (dvis_Plus/meta_architecture.py:1310-1311).  The same fp32 subtract and divide: same bits."""
    N, C, H, W = x.shape
    out = torch.empty((N, C, Hp, Wp), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        native.check(native.lib().dvis_normalize_pad(
            native.dev_ptr(x, "frames"), int(x.dtype == torch.uint8), native.dev_ptr(out, "out"), N * C, C, H, W, Hp, Wp,
            native.dev_ptr(mean.detach().reshape(-1), "pixel_mean"), native.dev_ptr(std.detach().reshape(-1), "pixel_std"),
            native.stream_ptr(x.device)), "dvis_normalize_pad")
    return out


def tokens_to_map(tokens, row0, h, w):
    """``tokens[:, row0 : row0 + h * w].transpose(1, 2).reshape(N, C, h, w)`` as a CONTIGUOUS map (tokens: (N, S, C) float32):
    one tiled transpose (dvis_tokens_to_nchw) instead of the strided view whose consumer copies it with torch's generic kernel
    (452 MB at the finest encoder level of 30 frames: 0.75 ms).  CPU / other dtypes / autograd: the view."""
    N, S, C = tokens.shape
    if not (tokens.is_cuda and tokens.dtype == torch.float32 and tokens.is_contiguous() and not torch.is_grad_enabled()):
        return tokens[:, row0:row0 + h * w].transpose(1, 2).reshape(N, C, h, w)
    out = torch.empty((N, C, h, w), dtype=torch.float32, device=tokens.device)
    with torch.cuda.device(tokens.device):
        native.check(native.lib().dvis_tokens_to_nchw(ctypes.c_void_p(tokens.data_ptr()), ctypes.c_void_p(out.data_ptr()), N, C, h * w,
                                                      S, row0, native.stream_ptr(tokens.device)), "dvis_tokens_to_nchw")
    return out


def conv1x1(x, weight, bias=None):
    """1x1 stride-1 convolution on NCHW.  On the GPU a channel-REDUCING 1x1 conv (Ci >= Co) is issued as the batched
    library GEMM W (Co,Ci) @ X (N,Ci,HW) instead of a MIOpen convolution: same contraction, same layout, measured on
    MI355X at the R50 / pixel-decoder shapes (tools/conv1x1_probe.py): 256->64 @184x320 1.10 -> 0.56 ms, 64->64
    0.55 -> 0.24 ms, 2048->256 0.32 -> 0.25 ms; channel-expanding ones are faster through MIOpen and stay there."""
    Co, Ci = weight.shape[:2]
    if conv1x1_x3_ok(x, weight):
        return conv1x1_x3(x, weight, bias)            # split-f16 matrix-core kernel (lateral / input / mask-feature projections)
    if bias is not None and CONV1X1_MFMA and x.is_cuda and x.dim() == 4 and x.is_contiguous() and x.dtype == torch.float32 \
            and weight.dtype == torch.float32 and not torch.is_grad_enabled() \
            and native.lib().dvis_conv1x1_mfma_supported(Ci, Co, x.shape[2] * x.shape[3]):
        return conv1x1_mfma(x, weight, bias)          # contraction + bias in one kernel (the pixel decoder's input projections)
    if x.is_cuda and Ci >= Co and x.is_contiguous() and x.dim() == 4 and x.dtype == weight.dtype \
            and not torch.is_grad_enabled():
        N, _, H, W = x.shape
        # bmm with a stride-0 batch of W, not torch.matmul: matmul folds the batch (transpose + copy of X, 4x slower)
        # whenever the 2-D operand is a Parameter that requires grad, even under no_grad
        y = torch.bmm(weight.detach().view(1, Co, Ci).expand(N, Co, Ci), x.view(N, Ci, H * W)).view(N, Co, H, W)
        return y if bias is None else bias_act_(y, bias.detach(), None, relu=False)   # in place, at the HBM stream rate
    # channel-expanding, strided (e.g. channels-last) or autograd inputs: MIOpen — a library call either way
    return torch.nn.functional.conv2d(x, weight, bias)


def conv1x1_bias_act(x, weight, bias=None, res=None, relu=False):
    """relu?(conv1x1(x, weight) + bias[c] + res) on NCHW.  Shapes dvis_conv1x1_bias_act serves (the memory-bound 1x1
    layers of the bottleneck at the large maps) run as ONE kernel — contraction and epilogue, no second pass over the
    output; every other shape is the library contraction followed by the in-place ``bias_act_`` pass."""
    Co, Ci = weight.shape[:2]
    if x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.is_contiguous() \
            and not torch.is_grad_enabled() and (res is None or (res.is_contiguous() and res.dtype == torch.float32)):
        N, _, H, W = x.shape
        if Ci >= X3_CONV1X1_MIN_CI and conv1x1_x3_ok(x, weight, 1, res):
            return conv1x1_x3(x, weight, bias, res, relu)
        if native.lib().dvis_conv1x1_supported(Ci, Co, H * W) and (res is None or res.shape == (N, Co, H, W)):
            w2 = weight.detach().reshape(Co, Ci)
            if not w2.is_contiguous():
                w2 = w2.contiguous()
            out = torch.empty((N, Co, H, W), dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device):
                rc = native.lib().dvis_conv1x1_bias_act(
                    native.dev_ptr(x, "x"), native.dev_ptr(w2, "weight"),
                    None if bias is None else native.dev_ptr(bias.detach(), "bias"),
                    None if res is None else native.dev_ptr(res, "res"), native.dev_ptr(out, "out"), N, Ci, Co, H * W,
                    1 if relu else 0, native.stream_ptr(x.device))
            native.check(rc, "dvis_conv1x1_bias_act")
            return out
        if CONV1X1_MFMA and native.lib().dvis_conv1x1_mfma_supported(Ci, Co, H * W) and (res is None or res.shape == (N, Co, H, W)):
            return conv1x1_mfma(x, weight, bias, res, relu)
    return bias_act_(conv1x1(x, weight), None if bias is None else bias.detach(), res, relu)


def conv1x1_x3_ok(x, weight, stride=1, res=None):
    """Does csrc/conv1x1_x3.hip (split-f16 matrix-core arithmetic, see csrc/gemm_x3.hip) serve this 1x1 convolution?"""
    if not (x3_on() and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.is_contiguous()
            and not torch.is_grad_enabled()):
        return False
    N, Ci, H, W = x.shape
    Co = weight.shape[0]
    OH, OW = (H + stride - 1) // stride, (W + stride - 1) // stride
    if res is not None and not (res.is_contiguous() and res.dtype == torch.float32 and tuple(res.shape) == (N, Co, OH, OW)):
        return False
    # (per IMAGE: a batch whose tensors exceed the kernel's 2 GiB of 32-bit offsets is launched in chunks of images by
    # _conv_x3_chunks — the dispatch, and with it a frame's bits, must not depend on how many frames share the call)
    return N == 0 or bool(native.lib().dvis_conv1x1_x3_supported(Ci, Co, 1, H * W, OH * OW))


def _conv_x3_chunks(N, Ci, Co, HW_in, HW_out):
    """Images per launch of the split-f16 convolution kernels: both tensors of a launch stay below 2 GiB."""
    per = max(Ci * HW_in, Co * HW_out) * 4
    return max(1, min(N, (2 ** 31 - 1) // per))


PD_GN_FOLD = os.environ.get("DVIS_PD_GN_FOLD", "1") != "0"


def gn_fold_ok(norm, K, HW):
    """May a split-f16 convolution with K output channels on maps of HW pixels leave the statistics of the GroupNorm `norm` behind
    (conv1x1_x3 / conv_x3_image, gn=norm)?  A wave's 32 pixels in one frame, a group = the 8 channels of one accumulator row pair."""
    return bool(PD_GN_FOLD and isinstance(norm, torch.nn.GroupNorm) and norm.num_channels == K
                and native.lib().dvis_conv_x3_gn_fold_supported(K, norm.num_groups, HW))


def affine_in_ok(x, weight):
    """May conv1x1_x3 apply a per-plane (scale, shift) (+ ReLU) to x as it reads it (affine=...)?  256 -> K % 256 == 0 channels, whole
    waves per frame."""
    return bool(PD_GN_FOLD and conv1x1_x3_ok(x, weight) and x.shape[1] == 256 and x.shape[0] > 0
                and native.lib().dvis_conv_x3_gn_fold_supported(weight.shape[0], weight.shape[0] // 8, x.shape[2] * x.shape[3]))


def _gn_partials(N, K, HW, device):
    """The side buffer of a gn= launch: (frame, group, 32-pixel slot, (sum, sum of squares)) in fp64, every element written."""
    return torch.empty((N, K // 8, HW // 32, 2), dtype=torch.float64, device=device)


def _gn_finalize(part, norm, N, K, HW):
    """group_norm_affine's (scale, shift) from the partial sums of a gn= launch."""
    scale = torch.empty(N * K, dtype=torch.float32, device=part.device)
    shift = torch.empty(N * K, dtype=torch.float32, device=part.device)
    with torch.cuda.device(part.device):
        native.check(native.lib().dvis_group_norm_finalize(
            native.dev_ptr(part, "partials"), None if norm.weight is None else native.dev_ptr(norm.weight.detach(), "gamma"),
            None if norm.bias is None else native.dev_ptr(norm.bias.detach(), "beta"), native.dev_ptr(scale, "scale"),
            native.dev_ptr(shift, "shift"), N, K, norm.num_groups, HW, float(norm.eps), native.stream_ptr(part.device)),
            "dvis_group_norm_finalize")
    return scale, shift


def conv1x1_x3(x, weight, bias=None, res=None, relu=False, stride=1, xexp=None, affine=None, affine_relu=False, gn=None):
    """relu?(conv1x1(x, weight)[:, :, ::stride, ::stride] + bias[c] + res) through dvis_conv1x1_x3.
    affine = (scale, shift) per plane of x (``group_norm_affine``): x is read as affine_relu?(x * scale + shift), the arithmetic of
    ``scale_shift_act_`` without its pass over the map (``affine_in_ok``).
    gn: a GroupNorm of the OUTPUT — returns (out, (scale, shift)) with the pair ``group_norm_affine(out, gn)`` returns, its
    statistics taken from the epilogue's registers where ``gn_fold_ok`` holds, by that kernel otherwise."""
    N, Ci, H, W = x.shape
    Co = weight.shape[0]

    def make():
        return _x3_pack_conv1x1(weight.detach().reshape(Co, Ci).contiguous())
    buf, wexp = _x3_cache(weight, [weight], make, kind="conv1x1")
    OH, OW = (H + stride - 1) // stride, (W + stride - 1) // stride
    out = torch.empty((N, Co, OH, OW), dtype=torch.float32, device=x.device)
    step = _conv_x3_chunks(N, Ci, Co, H * W, OH * OW)
    if affine is not None and not (affine_in_ok(x, weight) and stride == 1 and gn is None):
        raise RuntimeError("conv1x1_x3: this launch takes no input affine (see affine_in_ok); apply scale_shift_act_ first")
    part = _gn_partials(N, Co, OH * OW, x.device) if gn is not None and N > 0 and gn_fold_ok(gn, Co, OH * OW) else None
    with torch.cuda.device(x.device):
        for i in range(0, N, step):
            n = min(step, N - i)
            native.check(native.lib().dvis_conv1x1_x3(
                native.dev_ptr(x[i:i + n], "x"), ctypes.c_void_p(buf.data_ptr()),
                None if bias is None else native.dev_ptr(bias.detach(), "bias"),
                None if res is None else native.dev_ptr(res[i:i + n], "res"), native.dev_ptr(out[i:i + n], "out"), n, Ci, Co, H, W,
                stride, X3_CONV_XEXP if xexp is None else xexp, wexp, 1 if relu else 0, native.stream_ptr(x.device),
                None if affine is None else native.dev_ptr(affine[0].reshape(N, Ci)[i:i + n], "scale"),
                None if affine is None else native.dev_ptr(affine[1].reshape(N, Ci)[i:i + n], "shift"), 1 if affine_relu else 0,
                None if part is None else native.dev_ptr(part[i:i + n], "partials")), "dvis_conv1x1_x3")
    if gn is None:
        return out
    return out, (_gn_finalize(part, gn, N, Co, OH * OW) if part is not None else group_norm_affine(out, gn))


X3_DUAL = os.environ.get("DVIS_X3_DUAL", "1") != "0"


def conv1x1_x3_dual_ok(a, w3, x, ws, stride2):
    """conv3(a) + shortcut(x) of a bottleneck with a projection shortcut as ONE launch of the split-f16 kernel?"""
    if not (X3_DUAL and conv1x1_x3_ok(a, w3) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous()
            and ws.dtype == torch.float32 and ws.shape[0] == w3.shape[0] and stride2 in (1, 2)):
        return False
    N, C, H, W = a.shape
    N2, C2, H2, W2 = x.shape
    Co = w3.shape[0]
    return (N2 == N and C2 % 64 == 0 and 64 <= C2 <= 4096 and (H2 + stride2 - 1) // stride2 == H and (W2 + stride2 - 1) // stride2 == W
            and (C + C2) <= 4096 and bool(native.lib().dvis_conv1x1_x3_supported(C + C2, Co, 1, H * W, H * W))
            and C2 * H2 * W2 * 4 < 2 ** 31)


def conv1x1_x3_dual(a, w3, b3, x, ws, bs, relu=True, stride2=1, xexp=None):
    """relu?(conv1x1(a, w3) + b3 + conv1x1(x, ws)[:, :, ::stride2, ::stride2] + bs) through dvis_conv1x1_x3_dual."""
    N, C, H, W = a.shape
    _, C2, H2, W2 = x.shape
    Co = w3.shape[0]

    def make():
        wcat = torch.cat([w3.detach().reshape(Co, C), ws.detach().reshape(Co, C2)], 1).contiguous()
        buf, e = _x3_pack_conv1x1(wcat)
        bias = None
        if b3 is not None or bs is not None:
            bias = (0 if b3 is None else b3.detach()) + (0 if bs is None else bs.detach())
        return buf, e, bias
    buf, wexp, bias = _x3_cache(w3, [w3, ws, b3, bs], make, kind="conv1x1 + shortcut")
    out = torch.empty((N, Co, H, W), dtype=torch.float32, device=a.device)
    step = min(_conv_x3_chunks(N, C, Co, H * W, H * W), _conv_x3_chunks(N, C2, Co, H2 * W2, H * W))
    with torch.cuda.device(a.device):
        for i in range(0, N, step):
            n = min(step, N - i)
            native.check(native.lib().dvis_conv1x1_x3_dual(
                native.dev_ptr(a[i:i + n], "a"), native.dev_ptr(x[i:i + n], "x"), ctypes.c_void_p(buf.data_ptr()),
                None if bias is None else native.dev_ptr(bias, "bias"), None, native.dev_ptr(out[i:i + n], "out"), n, C, C2, Co, H, W,
                H2, W2, stride2, X3_CONV_XEXP if xexp is None else xexp, wexp, 1 if relu else 0, native.stream_ptr(a.device)),
                "dvis_conv1x1_x3_dual")
    return out


def conv3x3_x3_ok(x, weight, stride=1, res=None):
    """Does the 3x3 / padding 1 form of csrc/conv1x1_x3.hip serve this convolution?"""
    return weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3) and conv1x1_x3_ok(x, weight, stride, res)


def conv3x3_x3(x, weight, bias=None, res=None, relu=False, stride=1, xexp=None):
    """relu?(conv2d(x, weight, padding=1, stride=stride) + bias[c] + res) through dvis_conv3x3_x3."""
    N, Ci, H, W = x.shape
    Co = weight.shape[0]

    def make():
        return _x3_pack_conv3x3(weight.detach().contiguous())
    buf, wexp = _x3_cache(weight, [weight], make, kind="conv3x3")
    OH, OW = (H + stride - 1) // stride, (W + stride - 1) // stride
    out = torch.empty((N, Co, OH, OW), dtype=torch.float32, device=x.device)
    step = _conv_x3_chunks(N, Ci, Co, H * W, OH * OW)
    with torch.cuda.device(x.device):
        for i in range(0, N, step):
            n = min(step, N - i)
            native.check(native.lib().dvis_conv3x3_x3(
                native.dev_ptr(x[i:i + n], "x"), ctypes.c_void_p(buf.data_ptr()),
                None if bias is None else native.dev_ptr(bias.detach(), "bias"),
                None if res is None else native.dev_ptr(res[i:i + n], "res"), native.dev_ptr(out[i:i + n], "out"), n, Ci, Co, H, W,
                stride, X3_CONV_XEXP if xexp is None else xexp, wexp, 1 if relu else 0, native.stream_ptr(x.device)),
                "dvis_conv3x3_x3")
    return out


X3_IMAGES = os.environ.get("DVIS_X3_IMAGES", "1") != "0"


class OperandImage:
    """A C-channel map as csrc/conv1x1_x3.hip's operand image (include/dvis_hip.h: dvis_conv_x3_image): per 32-pixel group C / 64
    chunks of 8 KB of pre-split f16 terms.  `exp`: the power of two the values were scaled with before the split."""

    def __init__(self, data, N, C, H, W, exp):
        self.data, self.N, self.C, self.H, self.W, self.exp = data, N, C, H, W, exp

    @property
    def device(self):
        return self.data.device

    def images(self, i, n):
        per = self.data.numel() // self.N
        return self.data[i * per:(i + n) * per]


def x3_images_ok(N, C, K, H, W, device, taps=1, stride=1):
    """Operand images between two launches of csrc/conv1x1_x3.hip: split-f16 kernels on, a GPU, a 1x1 or 3x3 convolution (taps) of
    channel counts the image forms serve."""
    if not (X3_IMAGES and x3_on() and device.type == "cuda" and not torch.is_grad_enabled()):
        return False
    if taps not in (1, 9) or C % 64 != 0 or not (K == 128 or K % 256 == 0) or N <= 0:
        return False
    OH, OW = (H + stride - 1) // stride, (W + stride - 1) // stride
    return bool(native.lib().dvis_conv1x1_x3_supported(C, K, 1, H * W, OH * OW))


def _image_chunks(N, C, K, H, W, OH, OW):
    """Images per launch: every tensor of the launch below 2 GiB — fp32 maps, and operand images (rows padded to 32 pixels)."""
    per = max(C * H * ((W + 31) // 32 * 32), K * OH * ((OW + 31) // 32 * 32)) * 4
    return max(1, min(N, (2 ** 31 - 1) // per))


def _token_major_rows(top):
    """``top`` (N, C, h, w) as a view of token-major rows — ``tokens[:, r : r + h * w].transpose(1, 2).reshape(N, C, h, w)`` of an
    (N, S, C) tensor: S (h * w for a single frame), or 0 when it is anything else."""
    N, C, h, w = top.shape
    if not (top.stride(1) == 1 and top.stride(3) == C and top.stride(2) == w * C and top.data_ptr() % 16 == 0):
        return 0
    if N == 1:
        return h * w
    return top.stride(0) // C if top.stride(0) % C == 0 and top.stride(0) >= h * w * C else 0


def upsample_add_image_reads_tokens(lateral, top):
    """Does ``upsample_add_image`` read this ``top`` where it lies (dvis_upsample_add_image_tokens)?  A token-major view
    (``_token_major_rows``), a shape the second kernel form serves, and that form switched on (DVIS_UPSAMPLE_IMAGE_V2)."""
    N, C, H, W = lateral.shape
    lib = native.lib()
    return bool(lateral.is_cuda and top.is_cuda and top.dtype == torch.float32 and not top.is_contiguous() and _token_major_rows(top)
                and lateral.data_ptr() % 16 == 0 and lib.dvis_upsample_add_image_set_v2(-1)
                and lib.dvis_upsample_add_image_v2_supported(N, C, H, W, top.shape[-2], top.shape[-1]))


def upsample_add_image(lateral, top, lat_affine=None, oexp=None):
    """`upsample_add` with the sum written as an operand image (the 3x3 output convolution behind it reads fragments).  ``top``:
    an (N, C, h, w) map, or a token-major view of one (``upsample_add_image_reads_tokens``: read in place; any other strided
    view is copied)."""
    N, C, H, W = lateral.shape
    lib = native.lib()
    oe = X3_CONV_XEXP if oexp is None else oexp
    S = _token_major_rows(top) if upsample_add_image_reads_tokens(lateral, top) else 0
    if not S:
        top = top.contiguous()
    data = torch.empty(lib.dvis_conv_x3_image_bytes(N, C, H, W), dtype=torch.uint8, device=lateral.device)
    img = OperandImage(data, N, C, H, W, oe)
    step = _image_chunks(N, C, C, H, W, H, W)
    with torch.cuda.device(lateral.device):
        for i in range(0, N, step):
            n = min(step, N - i)
            sc = None if lat_affine is None else native.dev_ptr(lat_affine[0].reshape(N, C)[i:i + n], "scale")
            sh = None if lat_affine is None else native.dev_ptr(lat_affine[1].reshape(N, C)[i:i + n], "shift")
            if S:
                native.check(lib.dvis_upsample_add_image_tokens(
                    native.dev_ptr(lateral[i:i + n], "lateral"), sc, sh, ctypes.c_void_p(top[i:i + n].data_ptr()), S, 0,
                    ctypes.c_void_p(img.images(i, n).data_ptr()), n, C, H, W, top.shape[-2], top.shape[-1], oe,
                    native.stream_ptr(lateral.device)), "dvis_upsample_add_image_tokens")
                continue
            native.check(lib.dvis_upsample_add_image(native.dev_ptr(lateral[i:i + n], "lateral"), sc, sh, native.dev_ptr(top[i:i + n], "top"),
                                                     ctypes.c_void_p(img.images(i, n).data_ptr()), n, C, H, W, top.shape[-2], top.shape[-1], oe,
                                                     native.stream_ptr(lateral.device)), "dvis_upsample_add_image")
    return img


def conv_x3_image(src, weight, bias=None, res=None, relu=False, stride=1, out_image=False, oexp=None, xexp=None, gn=None):
    """relu?(conv2d(src, weight, stride, padding = k // 2) + bias + res) through dvis_conv_x3_image: `src` an OperandImage or an
    (N, C, H, W) fp32 map (then out_image must be set), weight (K, C, 1, 1) or (K, C, 3, 3); returns an OperandImage (out_image) or
    the (N, K, OH, OW) fp32 map.  gn (image in, map out): as in ``conv1x1_x3`` — returns (out, (scale, shift))."""
    lib = native.lib()
    from_img = isinstance(src, OperandImage)
    if not (from_img or out_image):
        raise ValueError("conv_x3_image: neither side is an operand image")
    N, C, H, W = (src.N, src.C, src.H, src.W) if from_img else src.shape
    K, taps = weight.shape[0], weight.shape[2] * weight.shape[3]
    dev = weight.device

    def make():
        w2 = weight.detach().contiguous()
        if from_img:
            return _x3_packed(w2, lib.dvis_conv1x1_x3_packed_bytes(C, K) * taps, lambda e, buf, st: lib.dvis_conv_x3_pack_image(
                native.dev_ptr(w2, "weight"), K, C, taps, e, buf, st), "dvis_conv_x3_pack_image")
        return _x3_pack_conv1x1(w2.reshape(K, C)) if taps == 1 else _x3_pack_conv3x3(w2)
    kind = ("conv%dx%d" % ((1, 1) if taps == 1 else (3, 3))) + (" image-in" if from_img else "")
    buf, wexp = _x3_cache(weight, [weight], make, kind=kind)
    OH, OW = (H + stride - 1) // stride, (W + stride - 1) // stride
    xe = src.exp if from_img else (X3_CONV_XEXP if xexp is None else xexp)
    oe = X3_CONV_XEXP if oexp is None else oexp
    if out_image:
        out = OperandImage(torch.empty(lib.dvis_conv_x3_image_bytes(N, K, OH, OW), dtype=torch.uint8, device=dev), N, K, OH, OW, oe)
    else:
        out = torch.empty((N, K, OH, OW), dtype=torch.float32, device=dev)
    step = _image_chunks(N, C, K, H, W, OH, OW)
    if gn is not None and not (from_img and not out_image):
        raise ValueError("conv_x3_image: gn needs an operand image in and an fp32 map out")
    part = _gn_partials(N, K, OH * OW, dev) if gn is not None and N > 0 and gn_fold_ok(gn, K, OH * OW) else None
    with torch.cuda.device(dev):
        for i in range(0, N, step):
            n = min(step, N - i)
            native.check(lib.dvis_conv_x3_image(
                ctypes.c_void_p(src.images(i, n).data_ptr()) if from_img else None, None if from_img else native.dev_ptr(src[i:i + n], "x"),
                ctypes.c_void_p(buf.data_ptr()), None if bias is None else native.dev_ptr(bias.detach(), "bias"),
                None if res is None else native.dev_ptr(res[i:i + n], "res"), None if out_image else native.dev_ptr(out[i:i + n], "out"),
                ctypes.c_void_p(out.images(i, n).data_ptr()) if out_image else None, n, C, K, H, W, stride, taps, xe, wexp, oe, 1 if relu else 0,
                native.stream_ptr(dev), None if part is None else native.dev_ptr(part[i:i + n], "partials")), "dvis_conv_x3_image")
    if gn is None:
        return out
    return out, (_gn_finalize(part, gn, N, K, OH * OW) if part is not None else group_norm_affine(out, gn))


X3_BNECK = os.environ.get("DVIS_X3_BNECK", "1") != "0"


def bneck_stage_x3_ok(x, blocks):
    """Does csrc/bneck_x3.hip serve this stage?  `blocks`: per bottleneck a dict of FOLDED weights / shifts
    {w1, b1, w2, b2, w3, b3, ws, bs} (ws / bs None for an identity shortcut) — the res2 stage of the R50: 64 -> (64, 3x3 64, 256),
    stride 1, a projection shortcut in the first block only."""
    if not (X3_BNECK and x3_on() and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous()
            and not torch.is_grad_enabled() and len(blocks) >= 2 and x.shape[1] == 64 and x.shape[0] > 0):
        return False
    for i, b in enumerate(blocks):
        cin = 64 if i == 0 else 256
        if tuple(b["w1"].shape) != (64, cin, 1, 1) or tuple(b["w2"].shape) != (64, 64, 3, 3) or tuple(b["w3"].shape) != (256, 64, 1, 1):
            return False
        if (b["ws"] is not None) != (i == 0) or (i == 0 and tuple(b["ws"].shape) != (256, 64, 1, 1)):
            return False
        if any(b[k] is not None and (b[k].dtype != torch.float32 or b[k].device != x.device) for k in b):
            return False
    return bool(native.lib().dvis_bneck_x3_supported(1, x.shape[2], x.shape[3]))


def bneck_stage_x3(x, blocks, xexp=None):
    """The whole stage through dvis_conv1x1_x3_image (first conv1) + one dvis_bneck_x3 per block (conv2 -> conv3 + shortcut ->
    the next block's conv1); the 64-channel maps between the launches are operand images.  Returns the stage's output."""
    N, _, H, W = x.shape
    lib = native.lib()
    xe = X3_CONV_XEXP if xexp is None else xexp
    dev = x.device

    def packed_conv1():
        w = blocks[0]["w1"]

        return _x3_cache(w, [w], lambda: _x3_pack_conv1x1(w.detach().reshape(64, 64).contiguous()), kind="conv1x1")

    def packed_block(i):
        b, nxt = blocks[i], (blocks[i + 1] if i + 1 < len(blocks) else None)
        ws, w1n = b["ws"], (None if nxt is None else nxt["w1"])

        def make():
            w2 = b["w2"].detach().contiguous()
            w3 = b["w3"].detach().reshape(256, 64).contiguous()
            wsd = None if ws is None else ws.detach().reshape(256, 64).contiguous()
            w1d = None if w1n is None else w1n.detach().reshape(64, 256).contiguous()
            e2, e1 = _x3_wexp(w2), (0 if w1d is None else _x3_wexp(w1d))
            e3 = _x3_wexp(w3 if wsd is None else torch.cat([w3, wsd], 1))
            buf = torch.empty(lib.dvis_bneck_x3_packed_bytes(0 if w1d is None else 1, 0 if wsd is None else 1), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                native.check(lib.dvis_bneck_x3_pack(native.dev_ptr(w2, "w2"), native.dev_ptr(w3, "w3"),
                                                    None if wsd is None else native.dev_ptr(wsd, "ws"),
                                                    None if w1d is None else native.dev_ptr(w1d, "w1"), e2, e3, e1,
                                                    ctypes.c_void_p(buf.data_ptr()), native.stream_ptr(dev)), "dvis_bneck_x3_pack")
            b3 = b["b3"]
            if b["bs"] is not None:
                b3 = b["bs"].detach() if b3 is None else b3.detach() + b["bs"].detach()
            return buf, e2, e3, e1, (None if b3 is None else b3.detach().clone())      # (an own tensor, derived.py)
        return _x3_cache(b["w2"], [b["w2"], b["w3"], ws, w1n, b["b3"], b["bs"]], make, kind="bottleneck chain")

    img_bytes = lib.dvis_bneck_x3_image_bytes(N, H, W)
    imgs = [torch.empty(img_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
    ys = [torch.empty((N, 256, H, W), dtype=torch.float32, device=dev) for _ in range(min(2, len(blocks)))]
    step = max(1, min(N, (2 ** 31 - 1) // (256 * H * W * 4)))       # images per launch: every tensor below 2 GiB
    per_img = img_bytes // N

    def ptr(t):
        return None if t is None else native.dev_ptr(t.detach(), "shift")

    with torch.cuda.device(dev):
        for i0 in range(0, N, step):
            n = min(step, N - i0)
            isl = slice(i0 * per_img, (i0 + n) * per_img)
            buf1, e1 = packed_conv1()
            native.check(lib.dvis_conv1x1_x3_image(native.dev_ptr(x[i0:i0 + n], "x"), ctypes.c_void_p(buf1.data_ptr()), ptr(blocks[0]["b1"]),
                                                   ctypes.c_void_p(imgs[0][isl].data_ptr()), n, 64, H, W, xe, e1, xe, 1, native.stream_ptr(dev)),
                         "dvis_conv1x1_x3_image")
            for i, b in enumerate(blocks):
                buf, e2, e3, e1n, b3 = packed_block(i)
                last = i + 1 == len(blocks)
                y, yprev = ys[i % 2], ys[(i + 1) % 2]
                native.check(lib.dvis_bneck_x3(
                    ctypes.c_void_p(imgs[i % 2][isl].data_ptr()), None if i == 0 else native.dev_ptr(yprev[i0:i0 + n], "res"),
                    native.dev_ptr(x[i0:i0 + n], "x") if i == 0 else None, ctypes.c_void_p(buf.data_ptr()), ptr(b["b2"]), ptr(b3),
                    None if last else ptr(blocks[i + 1]["b1"]), native.dev_ptr(y[i0:i0 + n], "y"),
                    None if last else ctypes.c_void_p(imgs[(i + 1) % 2][isl].data_ptr()), n, H, W, xe, e2, e3, e1n, native.stream_ptr(dev)),
                    "dvis_bneck_x3")
    return ys[(len(blocks) - 1) % 2]


def _fp32_pack(weight, kind, numel, pack, name):
    """The fp32 kernels' transformed weights (`numel` floats through `pack(weight pointer, buffer pointer, stream)`), one per
    (weight, kind) in derived.TABLE."""
    def make():
        w = weight.detach().contiguous()
        uf = torch.empty(numel, dtype=torch.float32, device=w.device)
        with torch.cuda.device(w.device):
            native.check(pack(native.dev_ptr(w, "weight"), native.dev_ptr(uf, "uf"), native.stream_ptr(w.device)), name)
        return uf
    return derived.TABLE.get(weight, kind, [weight], make)


CONV1X1_MFMA = os.environ.get("DVIS_CONV1X1_MFMA", "1") != "0"


def conv1x1s2_supported(x, weight):
    """Is the stride-2 1x1 convolution of x (the shortcut of a down-sampling bottleneck) served by csrc/conv1x1_mfma.hip?"""
    N, Ci, H, W = x.shape
    return CONV1X1_MFMA and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and not torch.is_grad_enabled() \
        and bool(native.lib().dvis_conv1x1_mfma_supported(Ci, weight.shape[0], ((H + 1) // 2) * ((W + 1) // 2))) \
        and 2 * Ci * H * W * 4 < 2 ** 31


def conv1x1_mfma(x, weight, bias=None, res=None, relu=False, stride=1):
    """relu?(conv1x1(x, weight) + bias[c] + res) for the compute-bound 1x1 layers (csrc/conv1x1_mfma.hip: C % 128 == 0, K % 64 == 0):
    contraction, folded-BN shift, shortcut add and ReLU in one kernel instead of the library's batched GEMM + ``bias_act_``.
    stride=2: the same on x[:, :, ::2, ::2] (read in place)."""
    N, Ci, H, W = x.shape
    Co = weight.shape[0]
    uf = _fp32_pack(weight, "conv1x1 mfma", Co * Ci, lambda w, uf, st: native.lib().dvis_conv1x1_mfma_pack(w, uf, Co, Ci, st),
                    "dvis_conv1x1_mfma_pack")
    if stride == 2:
        out = torch.empty((N, Co, (H + 1) // 2, (W + 1) // 2), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            rc = native.lib().dvis_conv1x1s2_mfma(
                native.dev_ptr(x, "x"), native.dev_ptr(uf, "uf"), None if bias is None else native.dev_ptr(bias.detach(), "bias"),
                None if res is None else native.dev_ptr(res, "res"), native.dev_ptr(out, "out"), N, Ci, Co, H, W, 1 if relu else 0,
                native.stream_ptr(x.device))
        native.check(rc, "dvis_conv1x1s2_mfma")
        return out
    out = torch.empty((N, Co, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = native.lib().dvis_conv1x1_mfma(
            native.dev_ptr(x, "x"), native.dev_ptr(uf, "uf"), None if bias is None else native.dev_ptr(bias.detach(), "bias"),
            None if res is None else native.dev_ptr(res, "res"), native.dev_ptr(out, "out"), N, Ci, Co, H * W, 1 if relu else 0,
            native.stream_ptr(x.device))
    native.check(rc, "dvis_conv1x1_mfma")
    return out


WINOGRAD_DEFAULT = os.environ.get("DVIS_WINOGRAD", "1") != "0"


def _winograd_weights(weight):
    K, C = weight.shape[:2]
    return _fp32_pack(weight, "winograd", 16 * K * C, lambda w, uf, st: native.lib().dvis_conv3x3_winograd_pack(w, uf, K, C, st),
                      "dvis_conv3x3_winograd_pack")


S2_DEFAULT = os.environ.get("DVIS_CONV3X3S2", "1") != "0"


def _s2_weights(weight):
    K, C = weight.shape[:2]
    return _fp32_pack(weight, "conv3x3s2", 12 * K * C, lambda w, uf, st: native.lib().dvis_conv3x3s2_pack(w, uf, K, C, st),
                      "dvis_conv3x3s2_pack")


def _library_conv_bias_act(x, weight, bias, relu, stride, padding):
    """The library convolution, then the in-place ``bias_act_`` pass unless there is nothing to add."""
    y = torch.nn.functional.conv2d(x, weight, None, stride, padding)
    if bias is None and not relu:
        return y
    return bias_act_(y, None if bias is None else bias.detach(), None, relu)


def conv3x3s2_bias_act(x, weight, bias=None, relu=False, own=None):
    """relu?(conv2d(x, weight (K, C, 3, 3), stride 2, padding 1) + bias[k]) on NCHW.  own=True: the direct fp32-MFMA kernel
    (csrc/conv3x3s2.hip: 119 - 131 TFLOP/s at the R50 shapes, 1.4 - 1.65x the library + epilogue pass), raising when the
    shape is not served; own=None: that kernel where the shape is served; otherwise the library convolution followed by the
    in-place ``bias_act_`` pass."""
    N, C, H, W = x.shape
    K = weight.shape[0]
    if own is None and conv3x3_x3_ok(x, weight, 2):
        return conv3x3_x3(x, weight, bias, None, relu, 2)      # nine-tap split-f16 matrix-core kernel: 1.6 - 2.2x the one below
    ok = x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and tuple(weight.shape[1:]) == (C, 3, 3) \
        and not (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)) \
        and bool(native.lib().dvis_conv3x3s2_supported(C, K, H, W))
    if own and not ok:
        raise RuntimeError(f"conv3x3s2_bias_act(own=True): C={C} K={K} H={H} W={W} is not served (dvis_conv3x3s2_supported)")
    if ok and (own or (own is None and WINOGRAD_DEFAULT and S2_DEFAULT)):
        x = x if x.is_contiguous() else x.contiguous()
        uf = _s2_weights(weight)
        out = torch.empty((N, K, (H + 1) // 2, W // 2), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            rc = native.lib().dvis_conv3x3s2(
                native.dev_ptr(x, "x"), native.dev_ptr(uf, "uf"), None if bias is None else native.dev_ptr(bias.detach(), "bias"),
                native.dev_ptr(out, "out"), N, C, K, H, W, 1 if relu else 0, native.stream_ptr(x.device))
        native.check(rc, "dvis_conv3x3s2")
        return out
    return _library_conv_bias_act(x, weight, bias, relu, 2, 1)


def conv7x7s2_stem(x, weight, bias=None, relu=False, own=None):
    """relu?(conv2d(x (N, 3, H, W), weight (64, 3, 7, 7), stride 2, padding 3) + bias[k]): the ResNet stem convolution on the
    direct fp32-MFMA kernel (csrc/conv7x7s2.hip) where the shape is served (own=True: raise otherwise), else the library."""
    N, C, H, W = x.shape
    K = weight.shape[0]
    ok = x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and tuple(weight.shape) == (64, 3, 7, 7) \
        and not (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)) \
        and bool(native.lib().dvis_conv7x7s2_supported(C, K, H, W))
    if own and not ok:
        raise RuntimeError(f"conv7x7s2_stem(own=True): C={C} K={K} H={H} W={W} is not served (dvis_conv7x7s2_supported)")
    if ok and (own or (own is None and WINOGRAD_DEFAULT and S2_DEFAULT)):
        uf = _fp32_pack(weight, "conv7x7s2", 10240, native.lib().dvis_conv7x7s2_pack, "dvis_conv7x7s2_pack")
        x = x if x.is_contiguous() else x.contiguous()
        out = torch.empty((N, 64, H // 2, W // 2), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            rc = native.lib().dvis_conv7x7s2(native.dev_ptr(x, "x"), native.dev_ptr(uf, "uf"),
                                             None if bias is None else native.dev_ptr(bias.detach(), "bias"),
                                             native.dev_ptr(out, "out"), N, H, W, 1 if relu else 0, native.stream_ptr(x.device))
        native.check(rc, "dvis_conv7x7s2")
        return out
    return _library_conv_bias_act(x, weight, bias, relu, 2, 3)


def conv3x3_bias_act(x, weight, bias=None, relu=False, winograd=None):
    """relu?(conv2d(x, weight (K, C, 3, 3), stride 1, padding 1) + bias[k]) on NCHW.  Shapes dvis_conv3x3_winograd serves run
    as ONE own kernel — Winograd F(2x2, 3x3) on the fp32 matrix cores, bias / ReLU in its epilogue (csrc/winograd_conv.hip:
    the FPN output convolution and conv2 of the R50 bottlenecks); other shapes, and `winograd=False` / DVIS_WINOGRAD=0, are
    the library convolution followed by the in-place ``bias_act_`` pass."""
    if winograd is None and weight.shape[1] >= 128 and conv3x3_x3_ok(x, weight, 1):
        # nine taps on the f16 matrix cores with split operands: 27 / 16 of an fp32 matrix-core product per output, the fp32
        # Winograd kernel below 4 — 1.2 - 1.5x faster from 128 input channels on (64: the Winograd kernel wins)
        return conv3x3_x3(x, weight, bias, None, relu, 1)
    use = WINOGRAD_DEFAULT if winograd is None else winograd
    if use and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and weight.dtype == torch.float32 \
            and tuple(weight.shape[2:]) == (3, 3) and not (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)):
        N, C, H, W = x.shape
        K = weight.shape[0]
        served = weight.shape[1] == C and native.lib().dvis_conv3x3_winograd_supported(C, K, H, W)
        if winograd and not served:
            raise RuntimeError(f"conv3x3_bias_act(winograd=True): shape C={C} K={K} H={H} W={W} is not served "
                               "(dvis_conv3x3_winograd_supported)")
        if served:
            x = x if x.is_contiguous() else x.contiguous()
            uf = _winograd_weights(weight)
            out = torch.empty((N, K, H, W), dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device):
                rc = native.lib().dvis_conv3x3_winograd(
                    native.dev_ptr(x, "x"), native.dev_ptr(uf, "uf"),
                    None if bias is None else native.dev_ptr(bias.detach(), "bias"), native.dev_ptr(out, "out"), N, C, K, H, W,
                    1 if relu else 0, native.stream_ptr(x.device))
            native.check(rc, "dvis_conv3x3_winograd")
            return out
    return _library_conv_bias_act(x, weight, bias, relu, 1, 1)


def bias_act_(x, bias=None, res=None, relu=True):
    """In place: x = relu?(x + bias[c] + res) on an NCHW float32 tensor — one pass instead of torch's three kernels
    (conv bias add, residual add, ReLU).  Non-GPU / odd shapes use the torch ops."""
    N, C, H, W = x.shape
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
            and (res is None or (res.is_contiguous() and res.shape == x.shape and res.dtype == torch.float32))
            and not torch.is_grad_enabled()):
        _torch_path("bias_act_", x, "needs contiguous fp32 NCHW (and a matching residual)")
        if bias is not None:
            x = x + bias.view(1, -1, 1, 1)
        if res is not None:
            x = x + res
        return torch.relu_(x) if relu else x
    with torch.cuda.device(x.device):
        rc = native.lib().dvis_bias_act(native.dev_ptr(x, "x"), None if bias is None else native.dev_ptr(bias, "bias"),
                                        None if res is None else native.dev_ptr(res, "res"), N * C, C, H * W,
                                        1 if relu else 0, native.stream_ptr(x.device))
    native.check(rc, "dvis_bias_act")
    return x


# --- video metrics: integer counts over (T, H, W) id maps (csrc/video_metrics.hip) -----------------------------------------------
# Dispatch by device: GPU tensors run the kernel (or raise), CPU tensors take the bincount formulations of cpu_ops.py.  Inputs may
# be any integer dtype and layout; they are made contiguous int32 first (one copy when they are not already).
def _i32(t, name):
    if t.dtype.is_floating_point or t.dtype == torch.bool or t.is_complex():
        raise RuntimeError(f"{name} must be an integer map, got {t.dtype}")
    return t.to(torch.int32).contiguous()


def _same_device(*ts):
    devs = {t.device for t in ts}
    if len(devs) != 1:
        raise RuntimeError(f"video metrics: tensors on different devices {sorted(map(str, devs))}")
    return ts[0].is_cuda


def pan_pair_hist(gt, pred, gt_table, num_pred, check=True):
    """Per-frame (GT segment, predicted segment) pixel counts of a clip (see dvis_pan_pair_hist).  gt (T, H, W): raw GT ids
    (r + 256 g + 65536 b, 0 = VOID); pred (T, H, W): dense predicted ids 0..num_pred; gt_table: the video's GT ids, sorted,
    non-zero.  Returns int64 (T, Ng + 2, num_pred + 1): row 0 VOID, 1 + i gt_table[i], Ng + 1 ids not in the table.
    check: validate the table and raise when a prediction lies outside 0..num_pred (host syncs)."""
    if gt.shape != pred.shape or gt.dim() != 3:
        raise RuntimeError(f"pan_pair_hist: gt {tuple(gt.shape)} and pred {tuple(pred.shape)} must be the same (T, H, W)")
    table = gt_table.reshape(-1)
    if check and table.numel() and bool((table[1:] <= table[:-1]).any() or (table <= 0).any()):
        raise ValueError("pan_pair_hist: gt_table must be strictly increasing positive ids")
    if not _same_device(gt, pred, table):
        counts, bad = cpu_ops.pan_pair_hist(gt, pred, table, int(num_pred))
    else:
        T, H, W = gt.shape
        g, p, tb = _i32(gt, "gt"), _i32(pred, "pred"), _i32(table, "gt_table")
        counts = torch.empty((T, tb.numel() + 2, int(num_pred) + 1), dtype=torch.int64, device=g.device)
        badt = torch.empty((1,), dtype=torch.int64, device=g.device)
        with torch.cuda.device(g.device):
            rc = native.lib().dvis_pan_pair_hist(native.dev_ptr(g, "gt"), native.dev_ptr(p, "pred"),
                                                 native.dev_ptr(tb, "gt_table") if tb.numel() else None, tb.numel(),
                                                 int(num_pred), T, H * W, native.dev_ptr(counts, "out"),
                                                 native.dev_ptr(badt, "bad"), native.stream_ptr(g.device))
        native.check(rc, "dvis_pan_pair_hist")
        bad = int(badt.item()) if check else 0
    if check and bad:
        raise ValueError(f"pan_pair_hist: {bad} predicted pixels outside 0..{num_pred}")
    return counts


def sem_confusion(gt, pred, num_class, check=True):
    """Class confusion (num_class, num_class) int64 of eval_miou_vspw.py:_generate_matrix over all pixels of gt / pred (same
    shape): VSPW labels (0 -> 255, - 1 in uint8, rows >= num_class dropped).  check: raise when a pixel would fall outside the
    matrix (negative prediction, or a bin past num_class^2, where the reference's reshape fails)."""
    if gt.shape != pred.shape:
        raise RuntimeError(f"sem_confusion: gt {tuple(gt.shape)} and pred {tuple(pred.shape)} differ")
    if not _same_device(gt, pred):
        conf, bad = cpu_ops.sem_confusion(gt, pred, int(num_class))
    else:
        g, p = _i32(gt, "gt"), _i32(pred, "pred")
        conf = torch.empty((int(num_class), int(num_class)), dtype=torch.int64, device=g.device)
        badt = torch.empty((1,), dtype=torch.int64, device=g.device)
        with torch.cuda.device(g.device):
            rc = native.lib().dvis_sem_confusion(native.dev_ptr(g, "gt") if g.numel() else None,
                                                 native.dev_ptr(p, "pred") if p.numel() else None, g.numel(), int(num_class),
                                                 native.dev_ptr(conf, "out"), native.dev_ptr(badt, "bad"),
                                                 native.stream_ptr(g.device))
        native.check(rc, "dvis_sem_confusion")
        bad = int(badt.item()) if check else 0
    if check and bad:
        raise ValueError(f"sem_confusion: {bad} pixels fall outside the {num_class} x {num_class} matrix")
    return conf


def video_consistency(gt, pred, ks=(8, 16)):
    """eval_vc_vspw.py:get_common's counts for a (T, H, W) clip: (gt_const, both_const), each (len(ks), T) int64 — for window
    length ks[j] and start i < T - k (the reference's range), the pixels whose GT is constant over [i, i + k) and those whose
    prediction is constant there too.  Entries i >= T - k are zero."""
    if gt.shape != pred.shape or gt.dim() != 3:
        raise RuntimeError(f"video_consistency: gt {tuple(gt.shape)} and pred {tuple(pred.shape)} must be the same (T, H, W)")
    ks = [int(k) for k in ks]
    if not _same_device(gt, pred):
        return cpu_ops.video_consistency(gt, pred, ks)
    T, H, W = gt.shape
    g, p = _i32(gt, "gt"), _i32(pred, "pred")
    gc = torch.empty((len(ks), T), dtype=torch.int64, device=g.device)
    bc = torch.empty((len(ks), T), dtype=torch.int64, device=g.device)
    karr = (ctypes.c_int32 * len(ks))(*ks)
    with torch.cuda.device(g.device):
        rc = native.lib().dvis_video_consistency(native.dev_ptr(g, "gt") if g.numel() else None,
                                                 native.dev_ptr(p, "pred") if p.numel() else None, T, H * W,
                                                 ctypes.cast(karr, ctypes.c_void_p), len(ks), native.dev_ptr(gc, "gt_const"),
                                                 native.dev_ptr(bc, "both_const"), native.stream_ptr(g.device))
    native.check(rc, "dvis_video_consistency")
    return gc, bc


# --- VIS scoring: COCO RLE and track intersections (csrc/vis_metrics.hip) ----------------------------------------------------------
# Same dispatch: GPU tensors run the kernels (or raise), CPU tensors take cpu_ops.py.  Masks are bool / uint8 (non-zero = set);
# runs are int32 tensors holding COCO's uint32 run lengths (a frame has < 2^31 pixels), laid out per mask at run_off (N + 1) int64.
RLE_ROWS = 128                 # rows per chunk of the encode table (csrc/vis_metrics.hip kRows)


def _u8(masks, name, contiguous=True):
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)                          # same bytes, any strides
    elif masks.dtype != torch.uint8:
        raise RuntimeError(f"{name} must be bool or uint8 masks, got {masks.dtype}")
    return masks.contiguous() if contiguous else masks


def _tracks(masks, name):
    """(masks, track stride): each track's (T, ...) frames contiguous, the tracks at any stride (a frame slice of a clip)."""
    m = _u8(masks, name, contiguous=False)
    if m.shape[0] and not m[0].is_contiguous():
        m = m.contiguous()
    return m, m.stride(0)


def rle_encode(masks):
    """COCO RLE of (N, H, W) masks: (runs int32, run_off (N + 1) int64, area (N) int64), on the masks' device.  The runs of mask
    n are runs[run_off[n]:run_off[n + 1]] (column-major pixel order, zeros first)."""
    if masks.dim() != 3:
        raise RuntimeError(f"rle_encode: masks must be (N, H, W), got {tuple(masks.shape)}")
    if not masks.is_cuda:
        return cpu_ops.rle_encode(masks)
    m = _u8(masks, "masks")
    N, H, W = m.shape
    dev = m.device
    if N == 0:
        return (torch.empty((0,), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int64, device=dev),
                torch.empty((0,), dtype=torch.int64, device=dev))
    nch = (H + RLE_ROWS - 1) // RLE_ROWS
    trans = torch.empty((N, W, nch), dtype=torch.int64, device=dev)
    area = torch.empty((N,), dtype=torch.int64, device=dev)
    lib = native.lib()
    with torch.cuda.device(dev):
        st = native.stream_ptr(dev)
        mp = native.dev_ptr(m, "masks") if m.numel() else None
        rc = lib.dvis_rle_encode(mp, N, H, W, 0, native.dev_ptr(trans, "trans"), native.dev_ptr(area, "area"), None, None, None,
                                 None, st)
        native.check(rc, "dvis_rle_encode")
        incl = trans.view(-1).cumsum(0)
        toff = incl - trans.view(-1)
        moff = torch.empty((N + 1,), dtype=torch.int64, device=dev)
        moff[:N] = toff.view(N, -1)[:, 0]
        moff[N:] = incl[-1:]
        total = int(moff[N])                                     # host sync: sizes the outputs
        bnd = torch.empty((max(total, 1),), dtype=torch.int32, device=dev)
        runs = torch.empty((total + N,), dtype=torch.int32, device=dev)
        rc = lib.dvis_rle_encode(mp, N, H, W, 1, None, None, native.dev_ptr(toff, "toff"), native.dev_ptr(moff, "moff"),
                                 native.dev_ptr(bnd, "bnd"), native.dev_ptr(runs, "runs") if runs.numel() else None, st)
        native.check(rc, "dvis_rle_encode")
    return runs, moff + torch.arange(N + 1, device=dev), area


def rle_strings(runs, run_off):
    """COCO's compressed `counts` strings (cocoapi rleToString) of every mask: (chars uint8, str_off (N + 1) int64) — mask n's
    string is bytes(chars[str_off[n]:str_off[n + 1]])."""
    if not _same_device(runs, run_off):
        return cpu_ops.rle_strings(runs, run_off)
    r, ro = runs.to(torch.int32).contiguous(), run_off.to(torch.int64).contiguous()
    N = ro.numel() - 1
    dev = r.device
    lens = torch.empty((N,), dtype=torch.int64, device=dev)
    lib = native.lib()
    with torch.cuda.device(dev):
        st = native.stream_ptr(dev)
        rp = native.dev_ptr(r, "runs") if r.numel() else None
        rc = lib.dvis_rle_strings(rp, native.dev_ptr(ro, "run_off"), N, None, native.dev_ptr(lens, "lens") if N else None, None,
                                  st)
        native.check(rc, "dvis_rle_strings")
        str_off = torch.zeros((N + 1,), dtype=torch.int64, device=dev)
        str_off[1:] = lens.cumsum(0)
        chars = torch.empty((int(str_off[-1]),), dtype=torch.uint8, device=dev)
        if chars.numel():
            rc = lib.dvis_rle_strings(rp, native.dev_ptr(ro, "run_off"), N, native.dev_ptr(str_off, "str_off"), None,
                                      native.dev_ptr(chars, "chars"), st)
            native.check(rc, "dvis_rle_strings")
    return chars, str_off


def rle_decode(runs, run_off, H, W):
    """(N, H, W) uint8 0 / 1 masks from COCO runs (each mask's runs must sum to H * W; checked)."""
    if not _same_device(runs, run_off):
        return cpu_ops.rle_decode(runs, run_off, H, W)
    r, ro = runs.to(torch.int64), run_off.to(torch.int64).contiguous()
    N = ro.numel() - 1
    dev = r.device
    cum = r.cumsum(0)
    n_runs = ro[1:] - ro[:-1]
    if bool((n_runs < 1).any()):
        raise ValueError("rle_decode: every mask needs at least one run")
    before = torch.cat((cum.new_zeros(1), cum))[ro[:-1]]          # pixels of the masks before mask n
    if not torch.equal(cum[ro[1:] - 1] - before, torch.full_like(before, H * W)):
        raise ValueError(f"rle_decode: a mask's runs do not sum to {H} x {W}")
    ends = (cum - torch.repeat_interleave(before, n_runs)).to(torch.int32)
    out = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = native.lib().dvis_rle_decode(native.dev_ptr(ends, "ends") if N else None, native.dev_ptr(ro, "run_off"), N, H, W,
                                          native.dev_ptr(out, "out") if N else None, native.stream_ptr(dev))
    native.check(rc, "dvis_rle_decode")
    return out


def track_intersections(pred, gt, out=None):
    """(P, G) int64 I[p, g] = sum over frames of |pred[p, t] & gt[g, t]| for masks pred (P, T, H, W) and gt (G, T, H, W) (any
    (T, ...) frame shape, the same on both sides).  out: an int64 (P, G) table to add to (GPU) — frame chunks of one video."""
    if pred.shape[1:] != gt.shape[1:]:
        raise RuntimeError(f"track_intersections: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} frames differ")
    if not _same_device(pred, gt):
        res = cpu_ops.track_intersections(pred, gt)
        return res if out is None else out.add_(res)
    (a, sa), (b, sb) = _tracks(pred, "pred"), _tracks(gt, "gt")
    P, G, T = a.shape[0], b.shape[0], a.shape[1]
    hw = a[0, 0].numel() if P and T else (b[0, 0].numel() if G and T else 0)
    dev = a.device
    acc = out is not None
    if out is None:
        out = torch.zeros((P, G), dtype=torch.int64, device=dev)
    elif out.shape != (P, G) or out.dtype != torch.int64 or not out.is_contiguous() or out.device != dev:
        raise RuntimeError(f"track_intersections: out must be a contiguous int64 ({P}, {G}) table on {dev}")
    if P == 0 or G == 0 or T == 0 or hw == 0:
        return out
    gs = max(1, min(G, (65536 - (P + 1) * 128) // (128 + 4 * max(P, 1))))     # GT columns per launch within 64 KB of LDS
    if P and (P + 1) * 128 + 4 * P > 65536:
        raise RuntimeError(f"track_intersections: {P} predicted tracks exceed one launch's LDS")
    with torch.cuda.device(dev):
        st = native.stream_ptr(dev)
        for g0 in range(0, G, gs):
            g1 = min(G, g0 + gs)
            part = out if gs >= G else torch.empty((P, g1 - g0), dtype=torch.int64, device=dev)
            if acc and gs < G:
                part.copy_(out[:, g0:g1])
            rc = native.lib().dvis_track_intersections(
                ctypes.c_void_p(a.data_ptr()), sa, P, ctypes.c_void_p(b[g0].data_ptr()), sb, g1 - g0, T, hw,
                1 if acc else 0, native.dev_ptr(part, "out"), st)
            native.check(rc, "dvis_track_intersections")
            if gs < G:
                out[:, g0:g1] = part
    return out


# --- prediction files: segment stats and painted maps (csrc/pred_write.hip) -------------------------------------------------------
# Same dispatch: GPU tensors run the kernels (or raise), CPU tensors take cpu_ops.py.  Maps are (T, H, W) integer tensors, made
# contiguous int32 (and 16-byte aligned for the paint kernels) first.
def _i32_aligned(t, name):
    m = _i32(t, name)
    return m if m.data_ptr() % 16 == 0 else m.clone()


def pan_segment_stats(pan, n):
    """(stats, bad): stats (T, n + 1, 5) int64 = area, xmin, ymin, xmax, ymax of every id 0..n in every frame (inclusive pixel
    coordinates, all zero where the id has no pixel); bad = the number of pixels whose id lies outside 0..n (an int on the CPU, a
    one-element int64 tensor on the GPU, read without a host sync)."""
    if pan.dim() != 3:
        raise RuntimeError(f"pan_segment_stats: the map must be (T, H, W), got {tuple(pan.shape)}")
    n = int(n)
    if not pan.is_cuda:
        return cpu_ops.pan_segment_stats(pan, n)
    T, H, W = pan.shape
    m = _i32(pan, "pan")
    out = torch.empty((T, n + 1, 5), dtype=torch.int64, device=m.device)
    bad = torch.empty((1,), dtype=torch.int64, device=m.device)
    with torch.cuda.device(m.device):
        rc = native.lib().dvis_pan_segment_stats(native.dev_ptr(m, "pan") if m.numel() else None, T, H, W, n,
                                                 native.dev_ptr(out, "out"), native.dev_ptr(bad, "bad"),
                                                 native.stream_ptr(m.device))
    native.check(rc, "dvis_pan_segment_stats")
    return out, bad


def pan_paint_rgb(pan, lut):
    """(T, H, W, 3) uint8 RGB of a (T, H, W) id map: colour lut[id] (int32 0x00BBGGRR per id 0..len(lut) - 1), black for ids
    outside the table."""
    if pan.dim() != 3:
        raise RuntimeError(f"pan_paint_rgb: the map must be (T, H, W), got {tuple(pan.shape)}")
    if not _same_device(pan, lut):
        return cpu_ops.pan_paint_rgb(pan, lut)
    m, lt = _i32_aligned(pan, "pan"), _i32(lut.reshape(-1), "lut")
    out = torch.empty((*m.shape, 3), dtype=torch.uint8, device=m.device)
    if m.numel():
        with torch.cuda.device(m.device):
            rc = native.lib().dvis_pan_paint_rgb(native.dev_ptr(m, "pan"), m.numel(),
                                                 native.dev_ptr(lt, "lut") if lt.numel() else None, lt.numel(),
                                                 native.dev_ptr(out, "out"), native.stream_ptr(m.device))
        native.check(rc, "dvis_pan_paint_rgb")
    return out


def sem_paint(sem, lut):
    """(out, bad): out = uint8 lut[sem & 255] (same shape as sem), lut (256) int = the dataset id 0..255 of each class byte or -1;
    bad (256) int64 = per class byte, the pixels that had no mapping (written as 255)."""
    if lut.numel() != 256:
        raise RuntimeError(f"sem_paint: lut must have 256 entries, got {lut.numel()}")
    if not _same_device(sem, lut):
        return cpu_ops.sem_paint(sem, lut)
    m, lt = _i32_aligned(sem, "sem"), _i32(lut.reshape(-1), "lut")
    out = torch.empty(m.shape, dtype=torch.uint8, device=m.device)
    bad = torch.empty((256,), dtype=torch.int64, device=m.device)
    with torch.cuda.device(m.device):
        rc = native.lib().dvis_sem_paint(native.dev_ptr(m, "sem") if m.numel() else None, m.numel(), native.dev_ptr(lt, "lut"),
                                         native.dev_ptr(out, "out") if m.numel() else None, native.dev_ptr(bad, "bad"),
                                         native.stream_ptr(m.device))
    native.check(rc, "dvis_sem_paint")
    return out, bad


# --- test-time frame resize (csrc/frame_resize.hip) ------------------------------------------------------------------------------
# detectron2's ResizeTransform.apply_image = Pillow Image.resize(BILINEAR) on uint8 frames.  Pillow's 8-bit resample is integer
# fixed point over per-axis coefficient tables (Resample.c precompute_coeffs + normalize_coeffs_8bpc); resize_tables restates
# them in the same double arithmetic, and both the kernel and the CPU formulation take them from here.
_RESIZE_PRECISION = 22
_resize_dev_tables = {}
_resize_lock = threading.Lock()


def _resize_host_table(n_in, n_out):
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    rows = []
    for o in range(n_out):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = []
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - t if t < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        rows.append([xmin, xmax] + [int(0.5 + v * (1 << _RESIZE_PRECISION)) for v in w] + [0] * (ksize - xmax))
    return torch.tensor(rows, dtype=torch.int32)


def resize_tables(n_in, n_out, device=None):
    """(n_out, k + 2) int32 table of one axis of Pillow's BILINEAR resample of n_in -> n_out pixels: per output index the first
    input index, the number of taps and k fixed-point (2^22) coefficients, zero past the taps.  k = 2 * ceil(max(n_in / n_out, 1))
    + 1.  Cached per (n_in, n_out) and per device; callers must not modify it."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise RuntimeError(f"resize_tables: sizes must be positive, got {n_in} -> {n_out}")
    dev = torch.device(device) if device is not None else torch.device("cpu")
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (n_in, n_out, dev)
    tab = _resize_dev_tables.get(key)
    if tab is None:
        host = _resize_dev_tables.get((n_in, n_out, torch.device("cpu")))
        if host is None:
            host = _resize_host_table(n_in, n_out)
        tab = host if dev.type == "cpu" else host.to(dev)
        with _resize_lock:
            _resize_dev_tables.setdefault((n_in, n_out, torch.device("cpu")), host)
            tab = _resize_dev_tables.setdefault(key, tab)
    return tab


def resize_frames_u8(frames, size, reverse_channels=False):
    """(T, 3, h, w) uint8 CHW: every (H, W, 3) uint8 frame of `frames` (T, H, W, 3) resized to size = (h, w) exactly as
    Image.fromarray(frame).resize((w, h), Image.BILINEAR) does (byte-identical), channels reversed if reverse_channels
    (BGR <-> RGB, which commutes with the resize).  GPU tensors run csrc/frame_resize.hip (or raise), CPU tensors the torch
    formulation of cpu_ops.py over the same tables.  Frames taller than 100 x their width are rejected (Pillow resizes those in
    the other order)."""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
        raise RuntimeError(f"resize_frames_u8: frames must be a uint8 tensor, got "
                           f"{frames.dtype if torch.is_tensor(frames) else type(frames).__name__}")
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise RuntimeError(f"resize_frames_u8: frames must be (T, H, W, 3), got {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise RuntimeError("resize_frames_u8: frames must be contiguous")
    T, H, W, _ = frames.shape
    h, w = (int(v) for v in size)
    if T == 0 or H == 0 or W == 0:
        raise RuntimeError(f"resize_frames_u8: no pixels to resize, frames {tuple(frames.shape)}")
    if h < 1 or w < 1:
        raise RuntimeError(f"resize_frames_u8: the output size must be positive, got {(h, w)}")
    if H > 100 * W:
        raise RuntimeError(f"resize_frames_u8: frames of {H}x{W} (taller than 100 x their width) are not supported")
    if H * W * 3 >= 2 ** 31 or h * w * 3 >= 2 ** 31 or T > 65535:
        raise RuntimeError(f"resize_frames_u8: too large: T {T}, {H}x{W} -> {h}x{w}")
    xtab, ytab = resize_tables(W, w, frames.device), resize_tables(H, h, frames.device)
    if not frames.is_cuda:
        return cpu_ops.resize_frames_u8(frames, xtab, ytab, reverse_channels)
    x = frames if frames.data_ptr() % 16 == 0 else frames.clone()
    out = torch.empty((T, 3, h, w), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = native.lib().dvis_resize_frames_u8(native.dev_ptr(x, "frames"), T, H, W, native.dev_ptr(out, "out"), h, w,
                                                native.dev_ptr(xtab, "xtab"), xtab.shape[1] - 2,
                                                native.dev_ptr(ytab, "ytab"), ytab.shape[1] - 2, int(bool(reverse_channels)),
                                                native.stream_ptr(x.device))
    native.check(rc, "dvis_resize_frames_u8")
    return out


# --- set criterion: matching cost and point-sampled mask losses (csrc/criterion.hip) ---------------------------------------------
# Dispatch by device like every op here: a GPU tensor runs the HIP kernel or the call raises (DVIS_STRICT=0 opts out: the torch
# formulation then runs on the GPU), a CPU tensor takes cpu_ops.py.  Masks may be strided views (the decoders return such): ONE
# .contiguous() copy is made here, the kernels see contiguous maps.  Half / bf16 predictions are upcast to fp32 BEFORE sampling.
# Reproducible backward of the point losses: 1 = always, 0 = never, default = when torch.use_deterministic_algorithms(True) is set.
POINT_LOSS_BWD_DETERMINISTIC = os.environ.get("DVIS_POINT_LOSS_BWD_DETERMINISTIC")


def _unserved(op, x, why):
    """A GPU tensor the criterion kernels do not serve: raise under the strict default — with or without autograd, these kernels
    have a backward —, else (DVIS_STRICT=0) let the caller take the torch formulation."""
    if x.is_cuda and os.environ.get("DVIS_STRICT", "1") != "0":
        raise RuntimeError(f"DVIS_STRICT: {op} would run its torch formulation on a GPU tensor ({why}; shape "
                           f"{tuple(x.shape)}, dtype {x.dtype})")
    return True


def _pred_f32(x, op):
    """fp32 / fp16 / bf16 predictions -> fp32 (upcast before sampling); anything else is not served."""
    if x.dtype in (torch.float16, torch.bfloat16):
        return x.float(), True
    return x, x.dtype == torch.float32


def _target_maps(t, device):
    """Target masks -> (contiguous tensor the kernels read, is-bytes flag): bool / uint8 stay bytes, fp32 stays, the rest -> fp32."""
    if t.device != device:
        t = t.to(device)
    if t.dtype == torch.bool:
        return t.contiguous().view(torch.uint8), 1
    if t.dtype == torch.uint8:
        return t.contiguous(), 1
    return t.to(torch.float32).contiguous(), 0


def _coords_f32(c, device):
    return c.to(device=device, dtype=torch.float32).contiguous()


@fp32_island
def match_cost(pred_masks, tgt_masks, coords, logits, tgt_ids, cost_class=1.0, cost_mask=1.0, cost_dice=1.0,
               return_terms=False):
    """The matching cost of VideoHungarianMatcher / HungarianMatcher for one batch element (matcher.py:107-151).
    pred_masks (Q, T, H, W) or (Q, H, W) mask logits; tgt_masks (G, T, Ht, Wt) / (G, Ht, Wt) fp32, uint8 or bool, at their own size; coords (K, 2) or
    (1, K, 2) normalised (x, y) shared by all masks and frames; logits (Q, C); tgt_ids (G) integer class ids.
    -> C (Q, G) fp32 = cost_mask * m + cost_class * c + cost_dice * d  [, terms (3, Q, G) = (c, m, d) unweighted]."""
    if pred_masks.dim() == 3:
        pred_masks, tgt_masks = pred_masks[:, None], tgt_masks[:, None]
    if pred_masks.dim() != 4 or tgt_masks.dim() != 4 or pred_masks.shape[1] != tgt_masks.shape[1]:
        raise RuntimeError(f"match_cost: pred_masks {tuple(pred_masks.shape)} and tgt_masks {tuple(tgt_masks.shape)} must be "
                           "(Q, T, H, W) and (G, T, Ht, Wt)")
    Q, T, H, W = pred_masks.shape
    G, _, Ht, Wt = tgt_masks.shape
    coords = coords.reshape(-1, 2)
    K = coords.shape[0]
    if logits.dim() != 2 or logits.shape[0] != Q or tgt_ids.shape != (G,):
        raise RuntimeError(f"match_cost: logits {tuple(logits.shape)} / tgt_ids {tuple(tgt_ids.shape)} do not fit Q {Q}, G {G}")
    if K == 0 or T == 0 or H * W == 0 or Ht * Wt == 0:
        raise RuntimeError("match_cost: no sample points / empty maps")
    dev = pred_masks.device
    pred, served = _pred_f32(pred_masks.detach(), "match_cost")
    logits = logits.detach()
    if G == 0 or Q == 0:
        C = torch.zeros((Q, G), dtype=torch.float32, device=dev)
        return (C, torch.zeros((3, Q, G), dtype=torch.float32, device=dev)) if return_terms else C
    if not dev.type == "cuda" or (not served and _unserved("match_cost", pred_masks, "dtype not fp32 / fp16 / bf16")):
        c, m, d = cpu_ops.match_cost_terms(pred.to(torch.float32), tgt_masks.to(dev), coords.to(dev), logits.to(dev),
                                           tgt_ids.to(dev))
        C = cost_mask * m + cost_class * c + cost_dice * d
        return (C, torch.stack((c, m, d))) if return_terms else C
    pred = pred.contiguous()
    tgt, u8 = _target_maps(tgt_masks, dev)
    co, lg = _coords_f32(coords, dev), logits.to(device=dev, dtype=torch.float32).contiguous()
    ids = tgt_ids.to(device=dev, dtype=torch.int64).contiguous()
    C = torch.empty((Q, G), dtype=torch.float32, device=dev)
    terms = torch.empty((3, Q, G), dtype=torch.float32, device=dev) if return_terms else None
    ws = torch.empty((native.lib().dvis_match_cost_ws_bytes(Q, G, T, K) + 3) // 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = native.lib().dvis_match_cost(native.dev_ptr(pred, "pred_masks"), native.dev_ptr(tgt, "tgt_masks"), u8,
                                          native.dev_ptr(co, "coords"), native.dev_ptr(lg, "logits"),
                                          native.dev_ptr(ids, "tgt_ids"), Q, G, T, H, W, Ht, Wt, K, lg.shape[1], float(cost_class),
                                          float(cost_mask), float(cost_dice), native.dev_ptr(C, "C"),
                                          native.dev_ptr(terms, "terms") if return_terms else None,
                                          native.dev_ptr(ws, "ws"), native.stream_ptr(dev))
    native.check(rc, "dvis_match_cost")
    return (C, terms) if return_terms else C


@fp32_island
def point_sample(rows, coords):
    """detectron2's point_sample(input (R, 1, H, W), point_coords (R, P, 2), align_corners=False) for one-channel rows:
    rows (R, H, W) fp32 / fp16 / bf16 / uint8 / bool, coords (R, P, 2) -> (R, P) fp32.  No gradient."""
    if rows.dim() != 3 or coords.dim() != 3 or coords.shape[0] != rows.shape[0] or coords.shape[2] != 2:
        raise RuntimeError(f"point_sample: rows {tuple(rows.shape)} must be (R, H, W) and coords {tuple(coords.shape)} (R, P, 2)")
    R, H, W = rows.shape
    P = coords.shape[1]
    dev = rows.device
    rows = rows.detach()
    if H * W == 0:
        raise RuntimeError("point_sample: empty maps")
    byte = rows.dtype in (torch.bool, torch.uint8)
    x, served = (rows, True) if byte else _pred_f32(rows, "point_sample")
    if dev.type != "cuda" or (not served and _unserved("point_sample", rows, "dtype not served")):
        with torch.no_grad():
            return cpu_ops.point_sample_rows(x, coords.to(dev))
    x, u8 = _target_maps(x, dev)
    co = _coords_f32(coords, dev)
    out = torch.empty((R, P), dtype=torch.float32, device=dev)
    if R * P == 0:
        return out
    with torch.cuda.device(dev):
        rc = native.lib().dvis_point_sample_rows(native.dev_ptr(x, "rows"), u8, native.dev_ptr(co, "coords"), R, P, H, W,
                                                 native.dev_ptr(out, "out"), native.stream_ptr(dev))
    native.check(rc, "dvis_point_sample_rows")
    return out


def _losses_from_sums(sums, P, num_masks):
    loss_mask = (sums[:, 0] / P).sum() / num_masks
    loss_dice = (1.0 - (2.0 * sums[:, 1] + 1.0) / (sums[:, 2] + 1.0)).sum() / num_masks
    return loss_mask, loss_dice


class PointMaskLossFunction(Function):
    """(loss_mask, loss_dice) of sigmoid_ce_loss + dice_loss on point-sampled rows (criterion.py:21-67) on the HIP kernels;
    gradient to src only."""

    @staticmethod
    def forward(ctx, src, tgt, tgt_u8, coords, num_masks, deterministic):
        R, H, W = src.shape
        Ht, Wt = tgt.shape[1:]
        P = coords.shape[1]
        dev = src.device
        sums = torch.empty((R, 3), dtype=torch.float32, device=dev)
        if R:
            ws = torch.empty((native.lib().dvis_point_loss_ws_bytes(R) + 3) // 4, dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                rc = native.lib().dvis_point_loss_fwd(native.dev_ptr(src, "src"), native.dev_ptr(tgt, "tgt"), tgt_u8,
                                                      native.dev_ptr(coords, "coords"), R, P, H, W, Ht, Wt,
                                                      native.dev_ptr(sums, "sums"), native.dev_ptr(ws, "ws"),
                                                      native.stream_ptr(dev))
            native.check(rc, "dvis_point_loss_fwd")
        ctx.save_for_backward(src, tgt, coords, sums)
        ctx.args = (tgt_u8, float(num_masks), deterministic)
        return _losses_from_sums(sums, P, float(num_masks))

    @staticmethod
    @once_differentiable
    def backward(ctx, g_mask, g_dice):
        src, tgt, coords, sums = ctx.saved_tensors
        tgt_u8, num_masks, deterministic = ctx.args
        R, H, W = src.shape
        Ht, Wt = tgt.shape[1:]
        P = coords.shape[1]
        dev = src.device
        grad = torch.empty_like(src)
        if R:
            gm = g_mask.to(torch.float32).reshape(1).contiguous()
            gd = g_dice.to(torch.float32).reshape(1).contiguous()
            if deterministic is None:
                deterministic = (POINT_LOSS_BWD_DETERMINISTIC == "1") if POINT_LOSS_BWD_DETERMINISTIC in ("0", "1") \
                    else torch.are_deterministic_algorithms_enabled()
            acc = torch.empty((R * H * W,), dtype=torch.int64, device=dev) if deterministic else None
            with torch.cuda.device(dev):
                rc = native.lib().dvis_point_loss_bwd(native.dev_ptr(src, "src"), native.dev_ptr(tgt, "tgt"), tgt_u8,
                                                      native.dev_ptr(coords, "coords"), native.dev_ptr(sums, "sums"),
                                                      native.dev_ptr(gm, "g_mask"), native.dev_ptr(gd, "g_dice"), R, P, H, W,
                                                      Ht, Wt, num_masks, native.dev_ptr(grad, "grad_src"),
                                                      native.dev_ptr(acc, "det_ws") if deterministic else None,
                                                      native.stream_ptr(dev))
            native.check(rc, "dvis_point_loss_bwd")
        return grad, None, None, None, None, None


@fp32_island
def point_mask_losses(src, tgt, coords, num_masks, deterministic=None):
    """loss_mask = sum_r mean_p bce(x, t) / num_masks and loss_dice = sum_r (1 - (2 a + 1) / (b + 1)) / num_masks of the matched
    rows: src (R, H, W) mask logits (fp32; fp16 / bf16 are upcast before sampling), tgt (R, Ht, Wt) fp32 / uint8 / bool (its own size),
    coords (R, P, 2) normalised (x, y) per row, num_masks a positive float.  Differentiable in src only.  Two 0-d tensors, formed
    on the device without a host sync.  deterministic: the backward's reproducible form (see POINT_LOSS_BWD_DETERMINISTIC)."""
    if src.dim() != 3 or tgt.dim() != 3 or tgt.shape[0] != src.shape[0] or coords.dim() != 3 or coords.shape[0] != src.shape[0] or coords.shape[2] != 2:
        raise RuntimeError(f"point_mask_losses: src {tuple(src.shape)}, tgt {tuple(tgt.shape)} must be (R, H, W), (R, Ht, Wt) and coords "
                           f"{tuple(coords.shape)} (R, P, 2)")
    num_masks = float(num_masks)
    P = coords.shape[1]
    if not num_masks > 0 or P == 0 or src.shape[1] * src.shape[2] == 0 or tgt.shape[1] * tgt.shape[2] == 0:
        raise RuntimeError("point_mask_losses: num_masks must be positive, P > 0 and the maps non-empty")
    dev = src.device
    x, served = _pred_f32(src, "point_mask_losses")
    if dev.type != "cuda" or (not served and _unserved("point_mask_losses", src, "dtype not fp32 / fp16 / bf16")):
        sums = cpu_ops.point_loss_sums(x.to(torch.float32), tgt.to(dev).detach(), coords.to(dev).detach())
        return _losses_from_sums(sums, P, num_masks)
    if src.shape[0] >= 65536:
        raise RuntimeError(f"point_mask_losses: {src.shape[0]} rows (at most 65535 per call)")
    t, u8 = _target_maps(tgt.detach(), dev)
    return PointMaskLossFunction.apply(x.contiguous(), t, u8, _coords_f32(coords.detach(), dev), num_masks, deterministic)


# --- contrastive item losses of CTVIS's CTCLPlugin (csrc/contrastive_items.hip) ---------------------------------------------------
# Item i = anchor row anchor[i] of src (R, C), positive rows pos_idx[pos_ptr[i]:pos_ptr[i + 1]], negative rows
# neg_idx[neg_ptr[i]:neg_ptr[i + 1]] (integer tensors; they originate on the host and are best handed over as CPU tensors: they
# are checked there, and GPU ones are copied back first).  Dispatch by device: a GPU tensor runs the kernels or the call raises, a
# CPU tensor takes cpu_ops.contrastive_items.  DVIS_CONTRASTIVE_ITEMS=0 selects the torch formulation on the GPU as well (timing
# tool and the tests' comparison).
def contrastive_items_transpose(anchor, pos_ptr, pos_idx, neg_ptr, neg_idx, R):
    """The backward's transposed incidence lists, built on the host from CPU index tensors (pure: no GPU, no library).
    -> (row_ptr (R + 1), occ_slot, occ_item, arow_ptr (R + 1), arow_item) int32: row r occurs as a positive / negative at
    occ_slot[row_ptr[r]:row_ptr[r + 1]] (global slot numbers: item i's slots start at pos_ptr[i] + neg_ptr[i], positives first) of the
    items occ_item[...], in (item, slot) order, and anchors the items arow_item[arow_ptr[r]:arow_ptr[r + 1]], ascending."""
    i64 = lambda t: torch.as_tensor(t).to(device="cpu", dtype=torch.int64)
    anchor, pos_ptr, pos_idx, neg_ptr, neg_idx = (i64(t) for t in (anchor, pos_ptr, pos_idx, neg_ptr, neg_idx))
    n = anchor.numel()
    items = torch.arange(n)
    P, N = pos_ptr[1:] - pos_ptr[:-1], neg_ptr[1:] - neg_ptr[:-1]
    base = pos_ptr[:-1] + neg_ptr[:-1]
    item_p, item_n = torch.repeat_interleave(items, P), torch.repeat_interleave(items, N)
    slot_p = base[item_p] + torch.arange(pos_idx.numel()) - pos_ptr[:-1][item_p]
    slot_n = base[item_n] + P[item_n] + torch.arange(neg_idx.numel()) - neg_ptr[:-1][item_n]
    rows, slots, item = torch.cat((pos_idx, neg_idx)), torch.cat((slot_p, slot_n)), torch.cat((item_p, item_n))
    S = max(int(slots.numel()), 1)
    order = torch.argsort(rows * S + slots)               # global slot numbers ascend with (item, slot)
    ptr = lambda r: torch.cat((torch.zeros(1, dtype=torch.int64), torch.bincount(r, minlength=R).cumsum(0)))
    a_order = torch.argsort(anchor, stable=True)
    i32 = lambda t: t.to(torch.int32)
    return i32(ptr(rows)), i32(slots[order]), i32(item[order]), i32(ptr(anchor)), i32(a_order)


class _ContrastiveItemLists:
    """The checked index lists of one call: host copies, the device copy (one upload), and on demand the transposed lists."""

    def __init__(self, op, R, anchor, pos_ptr, pos_idx, neg_ptr, neg_idx):
        lists = []
        for name, t in (("anchor", anchor), ("pos_ptr", pos_ptr), ("pos_idx", pos_idx), ("neg_ptr", neg_ptr), ("neg_idx", neg_idx)):
            t = torch.as_tensor(t)
            if t.dim() != 1 or t.dtype not in (torch.int32, torch.int64):
                raise RuntimeError(f"{op}: {name} must be a 1-d int32 / int64 tensor (got {tuple(t.shape)}, {t.dtype})")
            lists.append(t.detach().to(device="cpu", dtype=torch.int64))
        anchor, pos_ptr, pos_idx, neg_ptr, neg_idx = lists
        n = anchor.numel()
        for name, ptr, idx in (("pos", pos_ptr, pos_idx), ("neg", neg_ptr, neg_idx)):
            if ptr.numel() != n + 1 or int(ptr[0]) != 0 or int(ptr[-1]) != idx.numel() or bool((ptr[1:] < ptr[:-1]).any()):
                raise RuntimeError(f"{op}: {name}_ptr must have n + 1 = {n + 1} non-decreasing entries from 0 to len({name}_idx) = "
                                   f"{idx.numel()}")
        for name, idx in (("anchor", anchor), ("pos_idx", pos_idx), ("neg_idx", neg_idx)):
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= R):
                raise RuntimeError(f"{op}: {name} holds a row index outside [0, {R})")
        self.R, self.n, self.S, self.host = R, n, pos_idx.numel() + neg_idx.numel(), lists
        if self.S >= 2 ** 31 or R >= 2 ** 31:
            raise RuntimeError(f"{op}: {self.S} slots / {R} rows (fewer than 2^31 each)")
        self.dev = self.dev_t = None

    @staticmethod
    def _upload(parts, device):
        # every part starts on a 4-int boundary of ONE int32 buffer: one host-to-device copy
        sizes = [(p.numel() + 3) // 4 * 4 for p in parts]
        buf = torch.zeros(max(sum(sizes), 4), dtype=torch.int32)
        views, off = [], 0
        for p, s in zip(parts, sizes):
            buf[off:off + p.numel()] = p
            views.append((off, p.numel()))
            off += s
        buf = buf.to(device)
        return [buf[o:o + k] for o, k in views]

    def device(self, device):
        if self.dev is None:
            self.dev = self._upload(self.host, device)
        return self.dev

    def transposed(self, device):
        if self.dev_t is None:
            self.dev_t = self._upload(contrastive_items_transpose(*self.host, self.R), device)
        return self.dev_t


def _contrastive_items_iptr(view):
    """Device pointer of a slice of the uploaded index buffer (an EMPTY list still gets its place in the buffer, not null)."""
    return ctypes.c_void_p(view.untyped_storage().data_ptr() + 4 * view.storage_offset())


def _contrastive_items_src_check(op, src):
    if not (src.dim() == 2 and src.dtype == torch.float32 and src.is_contiguous() and src.shape[1] % 4 == 0 and src.shape[0] >= 1):
        raise RuntimeError(f"{op}: src must be a contiguous float32 (R, C) tensor with R >= 1 and C % 4 == 0 (got "
                           f"{tuple(src.shape)}, {src.dtype}, contiguous {src.is_contiguous()})")


def _contrastive_items_on_kernel(src):
    return src.is_cuda and os.environ.get("DVIS_CONTRASTIVE_ITEMS", "1") != "0"


def _contrastive_items_kernel(src, lists):
    """-> (reid (n), aux (n), saved = (dots (S), norms (S), stats (n, 3)))."""
    dev, n, S = src.device, lists.n, lists.S
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    reid, aux, dots, norms, stats = f(n), f(n), f(max(S, 1)), f(max(S, 1)), f(max(n, 1), 3)
    if n == 0:
        return reid, aux, (dots, norms, stats)
    d = lists.device(dev)
    with torch.cuda.device(dev):
        rc = native.lib().dvis_contrastive_items(
            native.dev_ptr(src, "src"), src.shape[0], src.shape[1], *(_contrastive_items_iptr(t) for t in d), n, S,
            native.dev_ptr(reid, "reid"), native.dev_ptr(aux, "aux"), native.dev_ptr(dots, "dots"), native.dev_ptr(norms, "norms"),
            native.dev_ptr(stats, "stats"), native.stream_ptr(dev))
    native.check(rc, "dvis_contrastive_items")
    return reid, aux, (dots, norms, stats)


def _contrastive_items_backward_kernel(src, lists, saved, grad_reid, grad_aux):
    dev, n, S = src.device, lists.n, lists.S
    R, C = src.shape
    if n == 0:
        return torch.zeros_like(src)
    dots, norms, stats = saved
    g = [t.detach().to(device=dev, dtype=torch.float32).expand(n).contiguous() for t in (grad_reid, grad_aux)]
    if not (dots.is_cuda and dots.numel() >= S and norms.numel() >= S and stats.numel() >= 3 * n):
        raise RuntimeError("contrastive_items_backward: `saved` is not what contrastive_items(..., return_saved=True) returned for these lists")
    lib = native.lib()
    grad_src = torch.empty_like(src)
    ws = torch.empty((max(lib.dvis_contrastive_items_backward_ws_bytes(n, S, C), 16) // 4,), dtype=torch.float32, device=dev)
    d, t = lists.device(dev), lists.transposed(dev)
    with torch.cuda.device(dev):
        rc = lib.dvis_contrastive_items_backward(
            native.dev_ptr(src, "src"), R, C, *(_contrastive_items_iptr(t) for t in d), n, S,
            *(_contrastive_items_iptr(x) for x in t), native.dev_ptr(dots, "dots"),
            native.dev_ptr(norms, "norms"), native.dev_ptr(stats, "stats"), native.dev_ptr(g[0], "grad_reid"),
            native.dev_ptr(g[1], "grad_aux"), native.dev_ptr(grad_src, "grad_src"), native.dev_ptr(ws, "workspace"),
            native.stream_ptr(dev))
    native.check(rc, "dvis_contrastive_items_backward")
    return grad_src


def contrastive_items_backward(src, anchor, pos_ptr, pos_idx, neg_ptr, neg_idx, saved, grad_reid, grad_aux):
    """Backward of ``contrastive_items`` on the kernels: saved = the forward's (dots, norms, stats), grad_reid / grad_aux (n) ->
    grad_src (R, C).  Exact fp32 without atomics, the same bits on every call; rows that no item references get exactly 0."""
    _contrastive_items_src_check("contrastive_items_backward", src)
    if not src.is_cuda:
        raise RuntimeError("contrastive_items_backward: the explicit backward runs the kernels: src must be a GPU tensor")
    lists = _ContrastiveItemLists("contrastive_items_backward", src.shape[0], anchor, pos_ptr, pos_idx, neg_ptr, neg_idx)
    return _contrastive_items_backward_kernel(src.detach(), lists, saved, grad_reid, grad_aux)


class ContrastiveItemsFunction(Function):
    """``contrastive_items`` under autograd: the forward kernel saves one dot and one norm per slot and three floats per item (never
    a gather of rows); the transposed lists are built on the host while the forward runs."""

    @staticmethod
    def forward(ctx, src, lists):
        reid, aux, saved = _contrastive_items_kernel(src, lists)
        if lists.n:
            lists.transposed(src.device)
        ctx.save_for_backward(src, *saved)
        ctx.lists = lists
        return reid, aux

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_reid, grad_aux):
        src, *saved = ctx.saved_tensors
        return _contrastive_items_backward_kernel(src, ctx.lists, saved, grad_reid, grad_aux), None


def contrastive_items(src, anchor, pos_ptr, pos_idx, neg_ptr, neg_idx, return_saved=False):
    """Per-item contrastive losses (ctvis.py's loss_reid before the division by the item count): src (R, C) fp32 ->
    reid (n) = logsumexp over all (negative - positive) . anchor pairs and one 0, aux (n) = mean squared difference between
    F.normalize's cosine and the label (1 positive, 0 negative).  One kernel launch for all items; with grad enabled and a src that
    requires grad the call goes through ContrastiveItemsFunction.  n = 0: two empty vectors, nothing is launched.
    return_saved: also the kernels' saved tensors, for ``contrastive_items_backward`` (GPU, no autograd)."""
    if src.dim() == 2 and src.is_floating_point() and src.shape[0] >= 1 and not _contrastive_items_on_kernel(src) and not return_saved:
        lists = _ContrastiveItemLists("contrastive_items", src.shape[0], anchor, pos_ptr, pos_idx, neg_ptr, neg_idx)
        return cpu_ops.contrastive_items(src, *lists.host)
    _contrastive_items_src_check("contrastive_items", src)
    if not src.is_cuda:
        raise RuntimeError("contrastive_items: return_saved needs the kernels: src must be a GPU tensor")
    lists = _ContrastiveItemLists("contrastive_items", src.shape[0], anchor, pos_ptr, pos_idx, neg_ptr, neg_idx)
    if torch.is_grad_enabled() and src.requires_grad and not return_saved:
        return ContrastiveItemsFunction.apply(src, lists)
    reid, aux, saved = _contrastive_items_kernel(src.detach(), lists)
    return (reid, aux, saved) if return_saved else (reid, aux)
