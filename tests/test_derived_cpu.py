"""CPU: dvis_plus_amd/derived.py — the one staleness / refresh policy of every weight-derived tensor — and the sites whose
private keys it replaced (ConvBN.folded, vit_adapter._Folded, graphs.FusedKV / ConvAsGemm)."""
from types import SimpleNamespace

import pytest
import torch

from dvis_plus_amd import derived


def _counting(fn):
    calls = []

    def make():
        calls.append(1)
        return fn()
    return make, calls


def test_hit_returns_the_identical_object_without_calling_make():
    w = torch.randn(3, 4)
    make, calls = _counting(lambda: w * 2)
    d = derived.Derived()
    a = d.get([w], make)
    assert d.get([w], make) is a and len(calls) == 1
    assert d.get([w], make, extra=(1,)) is a and len(calls) == 2       # an extra is part of the key (same shape: same storage)


def test_in_place_update_is_remade_into_the_same_storage():
    w = torch.randn(3, 4)
    make, calls = _counting(lambda: w * 2)
    d = derived.Derived()
    a = d.get([w], make)
    ptr = a.data_ptr()
    w.add_(1)
    b = d.get([w], make)
    assert len(calls) == 2 and b is a and b.data_ptr() == ptr and torch.equal(b, w * 2)


def test_data_swap_is_followed_although_the_version_stays():
    p = torch.nn.Parameter(torch.randn(3, 4))
    make, calls = _counting(lambda: p.detach() * 2)
    d = derived.Derived()
    a = d.get([p], make)
    ptr, ver = a.data_ptr(), p._version
    p.data = torch.randn(3, 4)
    assert p._version == ver
    b = d.get([p], make)
    assert len(calls) == 2 and b.data_ptr() == ptr and torch.equal(b, p.detach() * 2)


def test_shape_change_replaces_the_storage():
    p = torch.nn.Parameter(torch.randn(3, 4))
    d = derived.Derived()
    a = d.get([p], lambda: p.detach() * 2)
    p.data = torch.randn(5, 4)
    b = d.get([p], lambda: p.detach() * 2)
    assert b is not a and b.shape == (5, 4) and torch.equal(b, p.detach() * 2)
    # ... and so does another dtype or memory layout of the same shape
    c = d.get([p], lambda: (p.detach() * 2).double(), extra=("f64",))
    assert c is not b and c.dtype == torch.float64
    q = torch.randn(2, 3, 4, 4)
    e = derived.Derived()
    f = e.get([q], lambda: q * 2)
    g = e.get([q], lambda: (q * 2).contiguous(memory_format=torch.channels_last), extra=("cl",))
    assert g is not f and g.is_contiguous(memory_format=torch.channels_last)


def test_none_sources_and_tuple_values_with_scalars():
    w, b = torch.randn(3, 4), None
    n = [0]

    def make():
        n[0] += 1
        return w * 2, n[0], None, (w + 1, "x")
    d = derived.Derived()
    v1 = d.get([w, b], make)
    assert v1[1] == 1 and v1[2] is None and d.get([w, b], make) is v1
    w.mul_(3)
    v2 = d.get([w, b], make)
    assert v2[1] == 2 and v2[2] is None and v2[3][1] == "x"                   # the scalar member is the new one ...
    assert v2[0] is v1[0] and v2[3][0] is v1[3][0]                             # ... the tensors kept their storage
    assert torch.equal(v2[0], w * 2) and torch.equal(v2[3][0], w + 1)
    b = torch.zeros(3)
    assert d.get([w, b], make)[1] == 3                                         # None -> a tensor: stale
    assert derived.fingerprint([w, None], ("a", 2))[1:] == (None, "a", 2)


def test_table_keeps_one_entry_per_object_and_kind_and_holds_the_object():
    t = derived.Table(cap=2)
    w = torch.randn(2, 2)
    a = t.get(w, "a", [w], lambda: w + 1)
    b = t.get(w, "b", [w], lambda: w + 2)
    assert a is not b and len(t) == 2 and t.get(w, "a", [w], lambda: 1 / 0) is a
    ent = t.entry(w, "a", [w], lambda: 1 / 0, note=lambda: 1 / 0)             # an existing entry: neither make nor note runs
    assert ent.value is a and ent.key_obj is w and ent.note is None
    w.add_(1)
    assert t.get(w, "a", [w], lambda: w + 1) is a and torch.equal(a, w + 1)
    t.get(w, "c", [w], lambda: w + 3)                                          # past the cap: the least recently used ("b") goes
    assert len(t) == 2 and (id(w), "b") not in t.d and (id(w), "a") in t.d


# ---------------------------------------------------------------------------------------------------------------- the sites
@pytest.mark.parametrize("source", ["weight", "norm.weight", "norm.bias", "norm.running_mean", "norm.running_var"])
def test_convbn_folded_follows_each_of_its_five_sources(source):
    from dvis_plus_amd.backbone import ConvBN
    torch.manual_seed(0)
    conv = ConvBN(4, 6, 3, padding=1)
    for name in ("weight", "bias", "running_mean", "running_var"):
        getattr(conv.norm, name).copy_(torch.rand(6) + 0.5)
    w0, b0 = (t.clone() for t in conv.folded())
    t = conv
    for part in source.split("."):
        t = getattr(t, part)
    with torch.no_grad():
        t.add_(1.0)
    w1, b1 = conv.folded()
    n = conv.norm
    scale = n.weight * (n.running_var + n.eps).rsqrt()
    assert torch.equal(w1, conv.weight.detach() * scale.reshape(-1, 1, 1, 1))
    assert torch.equal(b1, n.bias - n.running_mean * scale)
    assert not (torch.equal(w1, w0) and torch.equal(b1, b0))
    assert conv.is_folded_weight(w1) and not conv.is_folded_weight(conv.weight)


def test_layerscale_fold_follows_gamma_and_a_data_swap_of_the_weight():
    from dvis_plus_amd.vit_adapter import LayerScale, _Folded
    torch.manual_seed(0)
    lin, ls, f = torch.nn.Linear(4, 6), LayerScale(6, 0.5), _Folded()
    w, b = f.get(lin, ls)
    assert torch.equal(w, lin.weight.detach() * 0.5) and torch.equal(b, lin.bias.detach() * 0.5)
    with torch.no_grad():
        ls.gamma.mul_(3.0)
    w2, b2 = f.get(lin, ls)
    assert w2 is w and torch.equal(w2, lin.weight.detach() * 1.5) and torch.equal(b2, lin.bias.detach() * 1.5)
    ver = lin.weight._version
    lin.weight.data = torch.randn(6, 4)
    assert lin.weight._version == ver
    w3, _ = f.get(lin, ls)
    assert w3 is w and torch.equal(w3, lin.weight.detach() * 1.5)
    # no LayerScale: the plain weights, as own tensors (a refresh must not write through a view of the parameter)
    g = _Folded()
    w4, b4 = g.get(lin, torch.nn.Identity())
    assert torch.equal(w4, lin.weight) and torch.equal(b4, lin.bias) and w4.data_ptr() != lin.weight.data_ptr()
    with torch.no_grad():
        lin.weight.add_(1.0)
    ver = lin.weight._version
    assert g.get(lin, torch.nn.Identity())[0] is w4 and torch.equal(w4, lin.weight) and lin.weight._version == ver


def _fused_kv_want(rows, layers, C):
    attn = [l.multihead_attn for l in layers]
    if rows == "out":
        return torch.stack([a.out_proj.weight for a in attn]), torch.stack([a.out_proj.bias for a in attn])
    W, b = [a.in_proj_weight for a in attn], [a.in_proj_bias for a in attn]
    if rows == "k_v":
        return (torch.cat([w[C:2 * C] for w in W] + [w[2 * C:] for w in W]), torch.cat([x[C:2 * C] for x in b] + [x[2 * C:] for x in b]))
    sl = slice(C, None) if rows == "kv" else slice(0, C)
    return torch.cat([w[sl] for w in W]), torch.cat([x[sl] for x in b])


@pytest.mark.parametrize("rows", ["kv", "k_v", "q", "out"])
def test_fused_kv_keeps_its_storage_across_a_weight_change(rows):
    from dvis_plus_amd.graphs import FusedKV
    torch.manual_seed(0)
    C = 8
    layers = [SimpleNamespace(multihead_attn=torch.nn.MultiheadAttention(C, 2)) for _ in range(3)]
    for l in layers:
        torch.nn.init.normal_(l.multihead_attn.in_proj_bias)
        torch.nn.init.normal_(l.multihead_attn.out_proj.bias)
    kv = FusedKV(rows)
    W, b = kv.get(layers, C)
    for got, want in zip((W, b), _fused_kv_want(rows, layers, C)):
        assert torch.equal(got, want)
    assert kv.get(layers, C)[0] is W
    ptrs = (W.data_ptr(), b.data_ptr())
    with torch.no_grad():
        for p in layers[1].multihead_attn.parameters():
            p.add_(1.0)
    W2, b2 = kv.get(layers, C)
    assert (W2.data_ptr(), b2.data_ptr()) == ptrs
    for got, want in zip((W2, b2), _fused_kv_want(rows, layers, C)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("k", [1, 3])
def test_conv_as_gemm_keeps_its_storage_across_a_weight_change(k):
    from dvis_plus_amd.graphs import ConvAsGemm
    torch.manual_seed(0)
    conv, cg = torch.nn.Conv1d(4, 6, k), ConvAsGemm()
    want = lambda: conv.weight.detach().permute(0, 2, 1).reshape(6, -1)
    W = cg.get(conv)
    assert torch.equal(W, want()) and W.data_ptr() != conv.weight.data_ptr() and cg.get(conv) is W
    with torch.no_grad():
        conv.weight.mul_(2.0)
    ver = conv.weight._version
    W2 = cg.get(conv)
    assert W2.data_ptr() == W.data_ptr() and torch.equal(W2, want()) and conv.weight._version == ver
