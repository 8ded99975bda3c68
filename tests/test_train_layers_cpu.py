"""The decoder-side layer classes' ``train_forward`` against their own ``forward`` on CPU tensors: the two spellings of a layer
are the same function there, bit for bit, in the output and in the gradient with respect to every input.  No tolerance: the test
fails as soon as one spelling changes and the other does not."""
import pytest
import torch

from dvis_plus_amd import cpu_ops
from dvis_plus_amd.transformer_decoder import MLP, CrossAttentionLayer, FFNLayer, SelfAttentionLayer

C, HEADS, Q, B, KEYS, FFN = 32, 4, 5, 2, 7, 64


def attend(q, k, v):
    return cpu_ops.attention(q, k, v, HEADS)


def inputs(dtype, *shapes):
    g = torch.Generator().manual_seed(7)
    return [torch.randn(s, generator=g, dtype=torch.float64).to(dtype) for s in shapes]


def run(fn, *xs):
    """Output of fn on fresh leaves of xs and the gradients of a fixed linear functional of it with respect to each."""
    leaves = [x.clone().requires_grad_(True) for x in xs]
    out = fn(*leaves)
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64).to(out.dtype)
    return out.detach(), torch.autograd.grad((out * cot).sum(), leaves)


def same(layer_fn, train_fn, dtype, *xs):
    out, grads = run(layer_fn, *xs)
    out_t, grads_t = run(train_fn, *xs)
    assert out.dtype == out_t.dtype == dtype
    assert torch.equal(out, out_t)
    for i, (g, g_t) in enumerate(zip(grads, grads_t)):
        assert g.dtype == dtype and torch.equal(g, g_t), f"gradient of input {i}"


def make(cls, dtype, *args, **kwargs):
    torch.manual_seed(3)
    layer = cls(*args, **kwargs).to(dtype)
    for p in layer.parameters():          # biases and the LayerNorm's affine start at 0 / 1: move them off those values
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.5)
    return layer


DTYPES = [torch.float32, torch.float64]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_pos", [False, True])
def test_self_attention(dtype, with_pos):
    layer = make(SelfAttentionLayer, dtype, C, HEADS)
    tgt, pos = inputs(dtype, (Q, B, C), (Q, 1, C))
    if with_pos:
        same(lambda t, p: layer(t, query_pos=p), lambda t, p: layer.train_forward(t, attend, query_pos=p), dtype, tgt, pos)
    else:
        same(lambda t: layer(t), lambda t: layer.train_forward(t, attend), dtype, tgt)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_attention(dtype):
    layer = make(CrossAttentionLayer, dtype, C, HEADS)
    tgt, memory, pos, query_pos = inputs(dtype, (Q, B, C), (KEYS, B, C), (KEYS, 1, C), (Q, 1, C))
    same(lambda t, m, p, qp: layer(t, m, pos=p, query_pos=qp),
         lambda t, m, p, qp: layer.train_forward(t, t + qp, m + p, m, attend), dtype, tgt, memory, pos, query_pos)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ffn(dtype):
    layer = make(FFNLayer, dtype, C, FFN)
    same(layer, layer.train_forward, dtype, *inputs(dtype, (Q, B, C)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_mlp(dtype):
    layer = make(MLP, dtype, C, C, 16, 3)
    same(layer, layer.train_forward, dtype, *inputs(dtype, (B, Q, C)))
