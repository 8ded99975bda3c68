"""GPU: the split-f16 kernels at the edges of their operand window (tests/x3_profiles.py: the profiles, the error model and
its derivation; tests/test_x3_error_model_cpu.py: the same model against an emulation of the arithmetic).

Per kernel: in-window accuracy against fp64 inside the derived bound with a silent guard; the limit exactly where
csrc/x3_common.h puts it (65520 / 2^xexp refused and named by the guard, the fp32 value below it served); NaN / Inf operands never
laundered into finite numbers; run-to-run bits.  Each body prints its worst error / bound and error / S before it asserts."""
import copy
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import x3_profiles as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GELU_GAIN = 1.13          # max |gelu'(t)| = 1.1290 (at t = sqrt 2 ...): the Lipschitz constant the split's terms pass through


@pytest.fixture(autouse=True)
def _inference_mode_and_a_clean_guard():
    from dvis_plus_amd import functions as Fn
    with torch.no_grad():
        _drain(Fn)
        yield
        _drain(Fn)


def _drain(Fn):
    try:
        Fn.X3_GUARD.check_now(torch.device(DEV))
    except Fn.X3RangeError:
        pass


def _fn():
    from dvis_plus_amd import functions as Fn
    return Fn


class Case:
    """One front-end as a linear map of (x, W, b) on 2-D operands: x (M, K) rows (pixels), W (N, K taps), out (M_out, N)."""
    xexp_of = "X3_XEXP"
    gain = 1.0
    relu = False
    exact_zero = True         # a zero matrix gives bias (+ residual) bit for bit
    kind = r"kernel\]"

    def __init__(self, name, M, K, N, **kw):
        self.name, self.M, self.K, self.N = name, M, K, N
        self.__dict__.update(kw)

    @property
    def xexp(self):
        return getattr(_fn(), self.xexp_of)

    @property
    def KW(self):
        return self.K

    def op(self, x, W, b):
        return P.linear_op(x, W, b)

    def res(self, dtype=torch.float32):
        return None

    def post(self, y):
        return y.clamp_min(0) if self.relu else y

    def affected(self, rows):
        """Output rows that read any of the input rows in the bool mask `rows`."""
        ind = rows[:, None].expand(self.M, self.K).double()
        return self.op(ind, torch.ones(self.N, self.KW, dtype=torch.float64), None).sum(1) > 0


class Linear(Case):
    def __init__(self, name, M, K, N, form="plain", **kw):
        super().__init__(name, M, K, N, form=form, **kw)
        self.relu = form == "relu"
        if form == "gelu_res":
            self.gain, self.exact_zero = GELU_GAIN, False
        g = torch.Generator().manual_seed(M + N)
        self._res = torch.randn(M, N, generator=g) if form == "gelu_res" else None
        self._pos = torch.randn(M, K, generator=g) if form == "xadd" else None

    def res(self, dtype=torch.float32):
        return None if self._res is None else self._res.to(dtype)

    def post(self, y):
        if self.form == "gelu_res":
            return F.gelu(y) + self._res.to(y.dtype)
        return super().post(y)

    def run(self, x, W, b, xexp=None):
        Fn = _fn()
        if self.form == "xadd":
            # x is the operand the kernel must see: hand it over as raw + pos with an fp32 sum that is exactly x
            pos = self._pos.to(DEV)
            raw = x - pos
            same = (raw + pos) == x
            pos, raw = torch.where(same, pos, torch.zeros_like(pos)), torch.where(same, raw, x)
            return Fn.x3_linear(raw.view(1, self.M, self.K), W, b, xadd=pos, xexp=xexp).view(self.M, self.N)
        if self.form == "gelu_res":
            return Fn.x3_linear(x, W, b, act="gelu", residual=self._res.to(DEV), xexp=xexp)
        if self.form == "tile":
            assert Fn.x3_tile_ok(x, self.N, self.K)
            return Fn.x3_tile_linear(x, W, b, xexp=xexp)
        if self.form == "tile_image":
            return Fn.x3_tile_linear(Fn.x3_rows_image(x, xexp=xexp), W, b)
        assert Fn.x3_ok(x, self.N, self.K)
        return Fn.x3_linear(x, W, b, relu=self.relu, xexp=xexp)


class Conv(Case):
    xexp_of = "X3_CONV_XEXP"

    def __init__(self, name, NB, Ci, Co, H, W, taps=1, stride=1, relu=False, with_res=False, form="conv", **kw):
        super().__init__(name, NB * H * W, Ci, Co, NB=NB, H=H, W=W, taps=taps, stride=stride, form=form, **kw)
        self.relu = relu
        self.OH, self.OW = (H + stride - 1) // stride, (W + stride - 1) // stride
        self._res = torch.randn(NB * self.OH * self.OW, Co, generator=torch.Generator().manual_seed(H + W)) if with_res else None

    @property
    def KW(self):
        return self.K * self.taps

    def res(self, dtype=torch.float32):
        return None if self._res is None else self._res.to(dtype)

    def to_map(self, x):
        return x.view(self.NB, self.H, self.W, -1).permute(0, 3, 1, 2).contiguous()

    def rows_of(self, y):
        return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])

    def weight4(self, W):
        k = 3 if self.taps == 9 else 1
        return W.view(self.N, self.K, k, k)

    def op(self, x, W, b):
        k = 3 if self.taps == 9 else 1
        xm = self.to_map(x)
        if k == 1:
            xm = xm[:, :, ::self.stride, ::self.stride]
            return self.rows_of(F.conv2d(xm, self.weight4(W), b))
        return self.rows_of(F.conv2d(xm, self.weight4(W), b, self.stride, 1))

    def post(self, y):
        if self._res is not None:
            y = y + self._res.to(y.dtype)
        return y.clamp_min(0) if self.relu else y

    def run(self, x, W, b, xexp=None):
        Fn = _fn()
        xm, w4 = self.to_map(x), self.weight4(W).contiguous()
        r = None if self._res is None else self._res.to(DEV).view(self.NB, self.OH, self.OW, self.N).permute(0, 3, 1, 2).contiguous()
        if self.form == "image_out":
            from test_conv_image_gpu import decode
            assert Fn.x3_images_ok(self.NB, self.K, self.N, self.H, self.W, xm.device)
            # the output image has a window of its own: its exponent is chosen for the outputs this call produces
            # (from the finite operands: a planted NaN / Inf is not part of that choice)
            fin = [torch.nan_to_num(t, 0.0, 0.0, 0.0).double().cpu() for t in (xm, w4, b)]
            ymax = float(F.conv2d(*fin).abs().max())
            self.oexp = min(Fn.X3_CONV_XEXP, int(math.floor(math.log2(65504.0 / max(ymax, 1e-30)))))
            img = Fn.conv_x3_image(xm, w4, b, None, relu=self.relu, out_image=True, xexp=xexp, oexp=self.oexp)
            return self.rows_of(decode(img))
        if self.form == "image_in":
            img = Fn.upsample_add_image(xm, torch.zeros(self.NB, self.K, max(1, self.H // 2), max(1, self.W // 2), device=DEV), oexp=xexp)
            return self.rows_of(Fn.conv_x3_image(img, w4, b, r, relu=self.relu, stride=self.stride))
        if self.taps == 9:
            assert Fn.conv3x3_x3_ok(xm, w4, self.stride)
            return self.rows_of(Fn.conv3x3_x3(xm, w4, b, r, self.relu, self.stride, xexp=xexp))
        assert Fn.conv1x1_x3_ok(xm, w4, self.stride, r)
        return self.rows_of(Fn.conv1x1_x3(xm, w4, b, r, self.relu, self.stride, xexp=xexp))


class Dual(Conv):
    """conv1x1_x3_dual: relu(conv3(a) + b3 + shortcut(xs)[::s] + bs) — one accumulation over the concatenated channels.  The
    profile's (M, K) rows are cut into the C channels of `a` and, at the positions the stride keeps, the C2 channels of `xs`."""

    def __init__(self, name, NB, C, C2, Co, H, W, s2):
        super().__init__(name, NB, C + C2, Co, H, W, relu=True, form="dual")
        self.C, self.C2, self.s2 = C, C2, s2
        # 1536 channels are 96 sequential accumulations of a 16-deep matrix product into the fp32 accumulator (x3_common.h:
        # mma_item, one `acc[nb] = mfma(.., acc[nb])` chain per output): each rounds to 2^-24 of the running sum, which S bounds.
        # The fp32 library convolution sums in blocks and does not stand for that chain at this depth (x3_profiles.bound).
        self.acc_steps = (C + C2) // 16
        self.H2, self.W2 = (2 * H, 2 * W) if s2 == 2 else (H, W)

    def run(self, x, W, b, xexp=None):
        Fn = _fn()
        xm = self.to_map(x)
        a = xm[:, :self.C].contiguous()
        xs = torch.randn(self.NB, self.C2, self.H2, self.W2, generator=torch.Generator().manual_seed(5)).to(DEV)
        xs[:, :, ::self.s2, ::self.s2] = xm[:, self.C:]
        w3, ws = W[:, :self.C].reshape(self.N, self.C, 1, 1).contiguous(), W[:, self.C:].reshape(self.N, self.C2, 1, 1).contiguous()
        assert Fn.conv1x1_x3_dual_ok(a, w3, xs, ws, self.s2)
        return self.rows_of(Fn.conv1x1_x3_dual(a, w3, b, xs, ws, None, relu=True, stride2=self.s2, xexp=xexp))


CASES = [
    Linear("linear N128 M1", 1, 256, 128), Linear("linear N288 M129", 129, 256, 288),
    Linear("linear relu N128 M129", 129, 256, 128, form="relu"), Linear("linear relu N288 M1", 1, 256, 288, form="relu"),
    Linear("linear xadd N288 M129", 129, 256, 288, form="xadd"), Linear("linear gelu+res N256 M129", 129, 256, 256, form="gelu_res"),
    Linear("linear stream K192 N192 M129", 129, 192, 192),
    Linear("tile K512 N256 M257", 257, 512, 256, form="tile", kind=r"\[tile kernel\]"),
    Linear("tile row image K512 N256 M257", 257, 512, 256, form="tile_image", kind=r"\[tile kernel\]"),
    Conv("conv1x1 64-256 20x31 res relu", 2, 64, 256, 20, 31, relu=True, with_res=True, kind=r"\[conv1x1 kernel\]"),
    Conv("conv1x1 64-256 20x31", 2, 64, 256, 20, 31, kind=r"\[conv1x1 kernel\]"),
    Conv("conv1x1 s2 64-256 20x31", 2, 64, 256, 20, 31, stride=2, kind=r"\[conv1x1 kernel\]"),
    Dual("conv1x1 dual 512+1024-2048 6x10 s2", 1, 512, 1024, 2048, 6, 10, 2),
    Conv("conv3x3 64-64 17x23 relu", 2, 64, 64, 17, 23, taps=9, relu=True, kind=r"\[conv3x3 kernel\]"),
    Conv("conv3x3 64-64 17x23", 2, 64, 64, 17, 23, taps=9, kind=r"\[conv3x3 kernel\]"),
    Conv("image out 256-512 4x64 relu", 1, 256, 512, 4, 64, relu=True, form="image_out", oexp=None, exact_zero=False, kind=r"\[conv1x1 kernel\]"),
    Conv("image in 256-512 4x64", 1, 256, 512, 4, 64, form="image_in", kind=r"image-in kernel\]"),
]
IDS = [c.name.replace(" ", "_") for c in CASES]

IN_WINDOW = [(a, w, 0) for a in P.IN_WINDOW for w in ("xavier", "heavy_tail")] + \
            [("normal", "pow2_max", k) for k in P.POW2_K] + [("normal", w, 0) for w in ("zero_row", "zero", "subnormal_max", "tiny_max")]


def _operands(case, act, wname, k=0, xexp=None):
    x = P.profile(act, (case.M, case.K), case.xexp if xexp is None else xexp, 21)
    return x, P.weights(wname, case.N, case.KW, 22, k=k), P.bias(case.N, 23)


def _gpu(case, x, W, b, xexp=None):
    return case.run(x.to(DEV), W.to(DEV), b.to(DEV), xexp).cpu()


def _image_floor(case, ref64):
    """An operand image stores its values as two f16 terms at 2^oexp: 22 bits of each value, and the floor below 2^-(3 + oexp)."""
    if getattr(case, "form", "") != "image_out":
        return 0.0
    return 2.0 ** -22 * ref64.abs() + 2.0 ** -(25 + case.oexp)


def _model(case, x, W, b, xexp):
    """(fp64 result, elementwise bound, S): the bound of x3_profiles with e_ref measured on the fp32 torch formulation."""
    ref = case.post(case.op(x.double(), W.double(), b.double()))
    B0, S = P.bound(x, W, b, xexp, 0.0, op=case.op, gain=case.gain, acc_steps=getattr(case, "acc_steps", 0))
    r = case.res(torch.float64)
    if r is not None:
        S = S + r.abs()
    e_ref = float(((case.post(case.op(x, W, b)).double() - ref).abs() / S).max())
    return ref, B0 + 1.25 * e_ref * S + _image_floor(case, ref), S


def _report(case, what, got, ref, B, S):
    err = (got.double() - ref).abs()
    ratio, rel = float((err / B).max()), float((err / S).max())
    print(f"x3-range | {case.name} | {what} | err/bound {ratio:.3f} | err/S {rel:.2e}")
    return ratio


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_in_window_operands_stay_inside_the_model(case):
    Fn = _fn()
    worst = {}
    for act, wname, k in IN_WINDOW:
        x, W, b = _operands(case, act, wname, k)
        got = _gpu(case, x, W, b)
        Fn.X3_GUARD.check_now(torch.device(DEV))          # in-window operands leave the guard silent
        assert torch.isfinite(got).all(), (act, wname)
        ref, B, S = _model(case, x, W, b, case.xexp)
        what = f"{act} x {wname}{k if wname == 'pow2_max' else ''}"
        worst[what] = _report(case, what, got, ref, B, S)
        if wname in ("zero", "subnormal_max") and case.exact_zero:
            zero = torch.zeros_like(W)
            assert torch.equal(got, case.post(case.op(torch.zeros_like(x), zero, b))), what
        if act == "dominated" and wname == "heavy_tail":
            assert torch.equal(got, _gpu(case, x, W, b)), "run-to-run bits"
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


def _split_rows(case, x, name):
    rows = torch.zeros(case.M, dtype=torch.bool)
    for r, _, _ in P.plants(name, (case.M, case.K), 21):
        rows[r] = True
    return case.affected(rows)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_limit_is_where_the_header_says(case):
    """65520 / 2^xexp in one element: its rows are refused (non-finite, the guard names the layer), every other row keeps its
    bits, and one exponent lower the same operands are served inside the model."""
    Fn = _fn()
    x, W, b = _operands(case, "edge_out", "xavier")
    r, c, _ = P.plants("edge_out", (case.M, case.K), 21)[0]
    assert float(x[r, c]) == P.limit(case.xexp) == {4: 4095.0, 2: 16380.0}[case.xexp]
    hit = _split_rows(case, x, "edge_out")
    got = _gpu(case, x, W, b)
    with pytest.raises(Fn.X3RangeError, match=case.kind):
        Fn.X3_GUARD.check_now(torch.device(DEV))
    assert bool(hit.any()) and not torch.isfinite(got[hit]).any(), "a value of a refused row came out finite"
    clean = x.clone()
    clean[r, c] = 1.0
    want = _gpu(case, clean, W, b)
    Fn.X3_GUARD.check_now(torch.device(DEV))
    assert torch.equal(got[~hit], want[~hit])
    served = _gpu(case, x, W, b, case.xexp - 1)
    Fn.X3_GUARD.check_now(torch.device(DEV))
    ref, B, S = _model(case, x, W, b, case.xexp - 1)
    assert torch.isfinite(served).all() and _report(case, f"edge_out at xexp {case.xexp - 1}", served, ref, B, S) <= 1.0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_non_finite_operands_are_never_laundered(case):
    Fn = _fn()
    x, W, b = _operands(case, "nonfinite", "xavier")
    hit = _split_rows(case, x, "nonfinite")
    got = _gpu(case, x, W, b)
    with pytest.raises(Fn.X3RangeError, match=case.kind):
        Fn.X3_GUARD.check_now(torch.device(DEV))
    assert not torch.isfinite(got[hit]).any(), "a value of a row with a NaN / Inf operand came out finite"
    clean = torch.where(torch.isfinite(x), x, torch.ones_like(x))
    assert torch.equal(got[~hit], _gpu(case, clean, W, b)[~hit])
    # a NaN weight: today the pack accepts it (exponent 0) and the GUARD fires at run time, naming the layer; every output
    # feature it feeds is non-finite in every row
    x, W, b = _operands(case, "normal", "nan")
    n = P.nan_index(case.N, case.KW)[0]
    got = _gpu(case, x, W, b)
    with pytest.raises(Fn.X3RangeError, match=case.kind):
        Fn.X3_GUARD.check_now(torch.device(DEV))
    assert not torch.isfinite(got[:, n]).any()


RELU_CASES = [c for c in CASES if c.relu]


@pytest.mark.parametrize("case", RELU_CASES, ids=[c.name.replace(" ", "_") for c in RELU_CASES])
def test_the_guard_reads_the_value_before_the_relu(case):
    """A pre-activation of -inf (a bias of -inf on one output feature: no NaN anywhere) leaves a ReLU as a clean 0.  Only a guard
    that reads the value BEFORE the ReLU can see it — every other planted value of this file becomes a NaN, which the epilogues'
    ReLU keeps, so they cannot tell the two placements apart."""
    Fn = _fn()
    x, W, b = _operands(case, "normal", "xavier")
    n = case.N // 2 + 1
    bad = b.clone()
    bad[n] = float("-inf")
    got = _gpu(case, x, W, bad)
    with pytest.raises(Fn.X3RangeError, match=case.kind):
        Fn.X3_GUARD.check_now(torch.device(DEV))
    assert torch.equal(got[:, n], torch.zeros(got.shape[0]))
    want = _gpu(case, x, W, b)
    Fn.X3_GUARD.check_now(torch.device(DEV))
    keep = torch.arange(case.N) != n
    assert torch.equal(got[:, keep], want[:, keep])


def test_an_image_output_beyond_its_own_window_is_named_at_the_producer():
    """conv_x3_image(out_image=True) re-splits its OUTPUT at 2^oexp: a value at or beyond 65520 / 2^oexp is stored as (inf, -inf).
    The producing launch tags the guard (not the consumer that would read the image), and the stored value decodes non-finite."""
    Fn = _fn()
    from test_conv_image_gpu import decode
    case = next(c for c in CASES if getattr(c, "form", "") == "image_out")
    x, W, b = _operands(case, "normal", "xavier")
    xm, w4 = case.to_map(x).to(DEV), case.weight4(W).contiguous().to(DEV)
    ref = case.rows_of(F.conv2d(case.to_map(x).double(), case.weight4(W).double(), b.double())).clamp_min(0)
    oexp = int(math.ceil(math.log2(65520.0 / float(ref.max())))) + 1          # the largest outputs leave the window, by a factor 4 at most
    beyond = ref * 2.0 ** oexp >= 65520.0
    inside = ref * 2.0 ** oexp < 65000.0
    assert 0 < int(beyond.sum()) < beyond.numel() // 4
    img = Fn.conv_x3_image(xm, w4, b.to(DEV), None, relu=True, out_image=True, oexp=oexp)
    with pytest.raises(Fn.X3RangeError, match=r"\[conv1x1 kernel\]"):
        Fn.X3_GUARD.check_now(torch.device(DEV))
    got = case.rows_of(decode(img)).cpu()
    assert not torch.isfinite(got[beyond]).any() and torch.isfinite(got[inside]).all()
    img = Fn.conv_x3_image(xm, w4, b.to(DEV), None, relu=True, out_image=True, oexp=oexp - 3)
    Fn.X3_GUARD.check_now(torch.device(DEV))
    assert torch.isfinite(decode(img)).all()


def _ln_operands(act, wname, M=129, C=256):
    Fn = _fn()
    x = P.profile(act, (M, C), Fn.X3_XEXP, 31)
    g = torch.Generator().manual_seed(32)
    norm = nn.LayerNorm(C)
    norm.weight.copy_(1.0 + 0.3 * torch.randn(C, generator=g))
    norm.bias.copy_(0.2 * torch.randn(C, generator=g))
    return x, norm, torch.randn(M, C, generator=g)


def _ln_check(name, what, got, pre64, B, norm):
    ref = F.layer_norm(pre64, (pre64.shape[-1],), norm.weight.double(), norm.bias.double(), norm.eps)
    e_ln = float((F.layer_norm(pre64.float(), (pre64.shape[-1],), norm.weight, norm.bias, norm.eps).double() - ref).abs().max())
    Bn = P.ln_bound(pre64, B, norm.weight, norm.eps, e_ln)
    err = (got.double() - ref).abs()
    ratio = float((err / Bn).max())
    print(f"x3-range | {name} | {what} | err/bound {ratio:.3f} | max err {float(err.max()):.2e}")
    return ratio


LN_PAIRS = [(a, w) for a in P.IN_WINDOW for w in ("xavier", "heavy_tail")] + [("normal", w) for w in ("zero_row", "zero", "subnormal_max")]


def test_linear_ln_in_window_and_at_the_limit():
    Fn = _fn()
    dev = torch.device(DEV)
    worst = {}
    for act, wname in LN_PAIRS:
        x, norm, res = _ln_operands(act, wname)
        W, b = P.weights(wname, 256, 256, 33), P.bias(256, 34)
        nd = copy.deepcopy(norm).to(DEV)
        got = Fn.x3_linear_ln(x.to(DEV), W.to(DEV), b.to(DEV), res.to(DEV), nd).cpu()
        Fn.X3_GUARD.check_now(dev)
        assert torch.isfinite(got).all()
        pre = x.double() @ W.double().t() + b.double() + res.double()
        B0, S = P.bound(x, W, b, Fn.X3_XEXP, 0.0)
        S = S + res.double().abs()
        e_ref = float((((F.linear(x, W, b) + res).double() - pre).abs() / S).max())
        worst[f"{act} x {wname}"] = _ln_check("linear_ln C256 M129", f"{act} x {wname}", got, pre, B0 + 1.25 * e_ref * S, norm)
        if act == "dominated" and wname == "heavy_tail":
            assert torch.equal(got, Fn.x3_linear_ln(x.to(DEV), W.to(DEV), b.to(DEV), res.to(DEV), nd).cpu())
    assert all(v <= 1.0 for v in worst.values()), worst
    for act in ("edge_out", "nonfinite"):
        x, norm, res = _ln_operands(act, "xavier")
        W, b = P.weights("xavier", 256, 256, 33), P.bias(256, 34)
        nd = copy.deepcopy(norm).to(DEV)
        got = Fn.x3_linear_ln(x.to(DEV), W.to(DEV), b.to(DEV), res.to(DEV), nd).cpu()
        with pytest.raises(Fn.X3RangeError, match=r"\[linear kernel\]"):
            Fn.X3_GUARD.check_now(dev)
        hit = torch.zeros(129, dtype=torch.bool)
        for r, _, _ in P.plants(act, (129, 256), 31):
            hit[r] = True
        assert not torch.isfinite(got[hit]).any() and torch.isfinite(got[~hit]).all()
        clean = torch.where(torch.isfinite(x) & (x.abs() < P.limit(Fn.X3_XEXP)), x, torch.ones_like(x))
        assert torch.equal(got[~hit], Fn.x3_linear_ln(clean.to(DEV), W.to(DEV), b.to(DEV), res.to(DEV), nd).cpu()[~hit])


def _ffn(wname):
    l1, l2 = nn.Linear(256, 1024), nn.Linear(1024, 256)
    l1.weight.copy_(P.weights(wname, 1024, 256, 41))
    l2.weight.copy_(P.weights(wname, 256, 1024, 42))
    l1.bias.copy_(0.5 * P.bias(1024, 43))
    l2.bias.copy_(0.5 * P.bias(256, 44))
    return l1, l2


def test_ffn_ln_in_window_and_at_the_limit():
    """x + lin2(relu(lin1(x))) -> LayerNorm: the first layer's bound passes through the ReLU (1-Lipschitz) and |W2|, the second
    layer's model applies to the fp64 hidden activations at the hidden exponent, the sum goes through `ln_bound`."""
    Fn = _fn()
    dev = torch.device(DEV)
    worst = {}
    for act, wname in LN_PAIRS:
        x, norm, _ = _ln_operands(act, wname)
        l1, l2 = _ffn(wname)
        h64 = F.relu(x.double() @ l1.weight.double().t() + l1.bias.double())
        # the hidden activations have a window of their own (`hexp`): heavy-tailed weights push them far beyond 4095, so the
        # exponent is chosen for the fp64 hidden maximum, as a caller with such weights has to
        hexp = min(Fn.X3_XEXP, int(math.floor(math.log2(65504.0 / max(float(h64.max()), 1e-30)))) - 1)
        nd, d1, d2 = copy.deepcopy(norm).to(DEV), copy.deepcopy(l1).to(DEV), copy.deepcopy(l2).to(DEV)
        got = Fn.x3_ffn_ln(x.to(DEV), d1, d2, nd, hexp=hexp).cpu()
        Fn.X3_GUARD.check_now(dev)
        assert torch.isfinite(got).all()
        pre = x.double() + h64 @ l2.weight.double().t() + l2.bias.double()
        B1, S1 = P.bound(x, l1.weight, l1.bias, Fn.X3_XEXP, 0.0)
        e1 = float(((F.linear(x, l1.weight, l1.bias).double() - (x.double() @ l1.weight.double().t() + l1.bias.double())).abs() / S1).max())
        B1 = B1 + 1.25 * e1 * S1
        B2, S2 = P.bound(h64, l2.weight, l2.bias, hexp, 0.0)
        S2 = S2 + x.double().abs()
        e2 = float((((x + F.linear(h64.float(), l2.weight, l2.bias)).double() - pre).abs() / S2).max())
        B = B2 + 1.25 * e2 * S2 + B1 @ l2.weight.double().abs().t()
        worst[f"{act} x {wname}"] = _ln_check("ffn_ln C256 H1024 M129", f"{act} x {wname}", got, pre, B, norm)
        if act == "dominated":
            assert torch.equal(got, Fn.x3_ffn_ln(x.to(DEV), d1, d2, nd, hexp=hexp).cpu())
        if hexp < Fn.X3_XEXP:
            # ... and at the default hidden exponent the same pair is refused loudly, never served wrong
            out = Fn.x3_ffn_ln(x.to(DEV), d1, d2, nd).cpu()
            with pytest.raises(Fn.X3RangeError, match=r"\[ffn kernel\]"):
                Fn.X3_GUARD.check_now(dev)
            assert not torch.isfinite(out[(h64 >= P.limit(Fn.X3_XEXP)).any(1)]).any()
    assert all(v <= 1.0 for v in worst.values()), worst
    for act in ("edge_out", "nonfinite"):
        x, norm, _ = _ln_operands(act, "xavier")
        l1, l2 = _ffn("xavier")
        nd, d1, d2 = copy.deepcopy(norm).to(DEV), copy.deepcopy(l1).to(DEV), copy.deepcopy(l2).to(DEV)
        got = Fn.x3_ffn_ln(x.to(DEV), d1, d2, nd).cpu()
        with pytest.raises(Fn.X3RangeError, match=r"\[ffn kernel\]"):
            Fn.X3_GUARD.check_now(dev)
        hit = torch.zeros(129, dtype=torch.bool)
        for r, _, _ in P.plants(act, (129, 256), 31):
            hit[r] = True
        assert not torch.isfinite(got[hit]).any() and torch.isfinite(got[~hit]).all()
        clean = torch.where(torch.isfinite(x) & (x.abs() < P.limit(Fn.X3_XEXP)), x, torch.ones_like(x))
        assert torch.equal(got[~hit], Fn.x3_ffn_ln(clean.to(DEV), d1, d2, nd).cpu()[~hit])


def test_layer_norm_rows_image_feeds_the_tiled_gemm_inside_the_model():
    """layer_norm_rows_image -> x3_tile_linear: the GEMM's operand is the normalised row, so a `dominated` input becomes the row
    with one massive activation (sqrt C) next to values 2^-16 below it.  The operand's own fp32 rounding (measured on torch's
    fp32 layer_norm) enters through sum_k |W_nk|."""
    Fn = _fn()
    M, C, N = 257, 512, 256
    for act in ("dominated", "floor", "log_uniform"):
        x = P.profile(act, (M, C), Fn.X3_XEXP, 51)
        g = torch.Generator().manual_seed(52)
        norm = nn.LayerNorm(C)
        norm.weight.copy_(1.0 + 0.3 * torch.randn(C, generator=g))
        norm.bias.copy_(0.2 * torch.randn(C, generator=g))
        W, b = P.weights("xavier", N, C, 53), P.bias(N, 54)
        n64 = F.layer_norm(x.double(), (C,), norm.weight.double(), norm.bias.double(), norm.eps)
        e_ln = float((F.layer_norm(x, (C,), norm.weight, norm.bias, norm.eps).double() - n64).abs().max())
        nd = copy.deepcopy(norm).to(DEV)
        xd = x.to(DEV)
        assert Fn.layer_norm_rows_image_ok(xd, nd)
        got = Fn.x3_tile_linear(Fn.layer_norm_rows_image(xd, nd), W.to(DEV), b.to(DEV)).cpu()
        Fn.X3_GUARD.check_now(torch.device(DEV))
        ref = n64 @ W.double().t() + b.double()
        B0, S = P.bound(n64, W, b, Fn.X3_XEXP, 0.0)
        e_ref = float(((F.linear(n64.float(), W, b).double() - ref).abs() / S).max())
        B = B0 + 1.25 * e_ref * S + 1.25 * e_ln * W.double().abs().sum(1)
        err = (got.double() - ref).abs()
        print(f"x3-range | layer_norm_rows_image + tile C512 N256 M257 | {act} x xavier | err/bound {float((err / B).max()):.3f} | err/S {float((err / S).max()):.2e}")
        assert torch.isfinite(got).all() and float((err / B).max()) <= 1.0


BN_H, BN_W = 16, 50


def _bneck_blocks(wname, k=0):
    """Two res2-shaped blocks (the chain serves no fewer) with every weight drawn from the profile `wname`."""
    def w(co, ci, kk, seed):
        return P.weights(wname, co, ci * kk * kk, seed, k=k).view(co, ci, kk, kk).contiguous()
    out = []
    for i in range(2):
        cin = 64 if i == 0 else 256
        out.append(dict(w1=w(64, cin, 1, 81 + 10 * i), b1=0.3 * P.bias(64, 82 + 10 * i), w2=w(64, 64, 3, 83 + 10 * i), b2=0.3 * P.bias(64, 84 + 10 * i),
                        w3=w(256, 64, 1, 85 + 10 * i), b3=0.3 * P.bias(256, 86 + 10 * i), ws=w(256, 64, 1, 87) if i == 0 else None,
                        bs=0.3 * P.bias(256, 88) if i == 0 else None))
    return out


def _bneck_model(x, blocks, xe):
    """fp64 stage output, its elementwise bound and the largest activation.  Layer by layer: the model of x3_profiles on the
    layer's fp64 input (e_ref measured on the fp32 library convolution of the same operands), plus the bound of the input carried
    through |W| (ReLU is 1-Lipschitz); the maps between the layers are operand images, whose two terms ARE the next layer's split.
    conv3 + projection shortcut is one accumulation over the concatenated channels with one weight exponent; an identity
    shortcut adds the block input and its bound."""
    def layer(inp, Bin, w, b, pad, extra=None, Bextra=None):
        def op(xx, ww, bb):
            return F.conv2d(xx, ww, bb, padding=pad)
        ref = op(inp, w.double(), b.double())
        B0, S = P.bound(inp, w, b, xe, 0.0, op=op)
        lib = op(inp.float(), w, b).double()
        if extra is not None:
            ref, S, lib = ref + extra, S + extra.abs(), (op(inp.float(), w, b) + extra.float()).double()
        e_ref = float(((lib - ref).abs() / S).max())
        B = B0 + 1.25 * e_ref * S + op(Bin, w.double().abs(), None) + (0 if Bextra is None else Bextra)
        return ref.clamp_min(0), B
    cur, Bcur = x.double(), torch.zeros_like(x, dtype=torch.float64)
    amax = float(cur.abs().max())
    for blk in blocks:
        a1, B1 = layer(cur, Bcur, blk["w1"], blk["b1"], 0)
        a2, B2 = layer(a1, B1, blk["w2"], blk["b2"], 1)
        if blk["ws"] is not None:
            y, By = layer(torch.cat([a2, cur], 1), torch.cat([B2, Bcur], 1), torch.cat([blk["w3"], blk["ws"]], 1), blk["b3"] + blk["bs"], 0)
        else:
            y, By = layer(a2, B2, blk["w3"], blk["b3"], 0, extra=cur, Bextra=Bcur)
        amax = max(amax, float(a1.max()), float(a2.max()), float(y.max()))
        cur, Bcur = y, By
    return cur, Bcur, amax


def _bneck_run(x, blocks, xexp=None):
    Fn = _fn()
    dev_blocks = [{k: (None if v is None else v.to(DEV)) for k, v in b.items()} for b in blocks]
    xd = x.to(DEV)
    assert Fn.bneck_stage_x3_ok(xd, dev_blocks)
    return Fn.bneck_stage_x3(xd, dev_blocks, xexp=xexp).cpu()


def _bneck_input(act, xe):
    return P.profile(act, (BN_H * BN_W, 64), xe, 62).view(1, BN_H, BN_W, 64).permute(0, 3, 1, 2).contiguous()


def test_bneck_stage_in_window_stays_inside_the_model():
    """bneck_stage_x3 at (1, 16, 50), two blocks, every profile pair of the other kernels.  A pair whose fp64 activations leave
    the window somewhere inside the chain (heavy-tailed weights multiply up through six layers) must be REFUSED: the guard names
    the chain.  Every other pair stays inside the layer-by-layer model."""
    Fn = _fn()
    dev = torch.device(DEV)
    xe = Fn.X3_CONV_XEXP
    worst = {}
    for act, wname, k in IN_WINDOW:
        x, blocks = _bneck_input(act, xe), _bneck_blocks(wname, k)
        ref, B, amax = _bneck_model(x, blocks, xe)
        got = _bneck_run(x, blocks)
        what = f"{act} x {wname}{k if wname == 'pow2_max' else ''}"
        if amax >= P.limit(xe):
            with pytest.raises(Fn.X3RangeError, match=r"kernel\]"):
                Fn.X3_GUARD.check_now(dev)
            print(f"x3-range | bneck_stage_x3 (1, 16, 50) | {what} | activations reach {amax:.3g}: refused, guard named the chain")
            continue
        Fn.X3_GUARD.check_now(dev)
        assert torch.isfinite(got).all(), what
        err = (got.double() - ref).abs()
        worst[what] = float((err / B).max())
        print(f"x3-range | bneck_stage_x3 (1, 16, 50) | {what} | err/bound {worst[what]:.3f} | err/max|ref| {float(err.max()) / max(float(ref.max()), 1e-30):.2e}")
        if act == "dominated":
            assert torch.equal(got, _bneck_run(x, blocks))
    assert len(worst) >= 10, "too few pairs stayed in the window to say anything"
    assert all(v <= 1.0 for v in worst.values()), worst


def test_bneck_stage_refuses_the_limit_and_non_finite_inputs():
    """The chain's first operand at the limit / NaN / Inf: the guard names a layer of the chain, every output the value reaches (two
    3 x 3 layers: the 5 x 5 pixels around it, all channels) is non-finite, every other pixel keeps its bits, and one exponent
    lower the limit value is served inside the model."""
    Fn = _fn()
    dev = torch.device(DEV)
    xe = Fn.X3_CONV_XEXP
    blocks = _bneck_blocks("xavier")
    x = _bneck_input("normal", xe)
    py, px, ch = BN_H // 2, BN_W // 2, 5
    clean = x.clone()
    clean[0, ch, py, px] = 1.0
    want = _bneck_run(clean, blocks)
    Fn.X3_GUARD.check_now(dev)
    hit = torch.zeros(BN_H, BN_W, dtype=torch.bool)
    hit[py - 2:py + 3, px - 2:px + 3] = True
    for bad in (P.limit(xe), float("nan"), float("inf")):
        xb = x.clone()
        xb[0, ch, py, px] = bad
        out = _bneck_run(xb, blocks)
        with pytest.raises(Fn.X3RangeError, match=r"kernel\]"):
            Fn.X3_GUARD.check_now(dev)
        assert not torch.isfinite(out[0][:, hit]).any(), bad
        assert torch.equal(out[0][:, ~hit], want[0][:, ~hit]), bad
    xb = x.clone()
    xb[0, ch, py, px] = P.limit(xe)
    served = _bneck_run(xb, blocks, xexp=xe - 1)
    Fn.X3_GUARD.check_now(dev)
    ref, B, amax = _bneck_model(xb, blocks, xe - 1)
    ratio = float(((served.double() - ref).abs() / B).max())
    print(f"x3-range | bneck_stage_x3 (1, 16, 50) | limit value at xexp {xe - 1} | err/bound {ratio:.3f}")
    assert amax < P.limit(xe - 1) and torch.isfinite(served).all() and ratio <= 1.0
    xb[0, ch, py, px] = P.below_limit(xe)
    got = _bneck_run(xb, blocks)
    Fn.X3_GUARD.check_now(dev)
    ref, B, _ = _bneck_model(xb, blocks, xe)
    assert torch.isfinite(got).all() and float(((got.double() - ref).abs() / B).max()) <= 1.0


def test_qkv_attention_on_dominated_and_floor_rows():
    """x3_qkv_attention at B = 1, L = 1024, 8 heads of 64 (C = 512 is the narrowest projection the tiled kernel serves): rows with one massive activation and rows scaled down to 2^-24, at the
    tolerance of test_long_self_attention_on_split_f16_products_vs_fp64 (max(2 e_f32, 2e-5) against fp64, next to the exact
    path's own error); bits repeat; the limit in one token is named by the guard."""
    Fn = _fn()
    B_, L, heads, C = 1, 1024, 8, 512
    g = torch.Generator().manual_seed(71)
    w = torch.randn(3 * C, C, generator=g) * C ** -0.5
    b = torch.randn(3 * C, generator=g) * 0.1
    for act in ("dominated", "floor"):
        x = P.profile(act, (L, C), Fn.X3_XEXP, 72)
        if act == "dominated":
            w_use = w * 2.0 ** -6          # q k^T / 8 of a 3000-valued row stays a usable softmax logit
        else:
            w_use = w
        xd, wd, bd = x.view(B_, L, C).to(DEV), w_use.to(DEV), b.to(DEV)
        if not Fn.x3_qkv_attention_ok(xd, wd, heads):
            pytest.fail("x3_qkv_attention does not serve (1, 1024, 512)")
        out = Fn.x3_qkv_attention(xd, wd, bd, heads)
        Fn.X3_GUARD.check_now(torch.device(DEV))
        qkv = (x.double() @ w_use.double().t() + b.double()).view(B_, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
        ref = (torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) / 8.0, -1) @ qkv[2]).permute(0, 2, 1, 3).reshape(B_, L, C)
        with Fn.x3_disabled():
            q32 = Fn.linear(xd, wd, bd).transpose(0, 1)
            exact = torch.empty_like(out)
            Fn.attention(q32[..., :C], q32[..., C:2 * C], q32[..., 2 * C:], heads, out=exact.transpose(0, 1))
        e_x3, e_f32 = float((out.cpu().double() - ref).abs().max()), float((exact.cpu().double() - ref).abs().max())
        print(f"x3-range | x3_qkv_attention (1, 1024, 8 x 64) | {act} | max err {e_x3:.2e} | exact path {e_f32:.2e}")
        assert torch.isfinite(out).all() and e_x3 <= max(2.0 * e_f32, 2e-5), (act, e_x3, e_f32)
        assert torch.equal(out, Fn.x3_qkv_attention(xd, wd, bd, heads))
    x = P.profile("edge_out", (L, C), Fn.X3_XEXP, 72)
    out = Fn.x3_qkv_attention(x.view(B_, L, C).to(DEV), w.to(DEV), b.to(DEV), heads)
    with pytest.raises(Fn.X3RangeError, match=r"\[tile kernel\]"):
        Fn.X3_GUARD.check_now(torch.device(DEV))
    # the token's q, k and v are NaN: its own output row through q, every other row through k
    assert not torch.isfinite(out).any()
