"""functions.attention_plan / dvis_attention_plan: the attention dispatch at each of its thresholds, asked of the host function the
launch itself consults (no GPU: only shapes and strides are read).  The GPU files assert their cases' plans; this one pins where
the boundaries are."""
import pytest
import torch

FWD, SHORT, X3, KEYSPLIT = "attn_fwd_kernel", "attn_short_kernel", "attn_x3_kernel", "attn_keysplit_kernel"


def plan(Lq, Lk, d=32, masked=False, short=False, B=2, H=2):
    from dvis_plus_amd import functions as Fn
    q, k = torch.empty(Lq, B, H * d), torch.empty(Lk, B, H * d)
    mask = torch.empty(B, Lq, Lk, dtype=torch.uint8) if masked else None
    return Fn.attention_plan(q, k, H, mask, short)


@pytest.mark.parametrize("args,kernel", [
    ((100, 128, 32), SHORT), ((100, 129, 32), FWD), ((100, 128, 64), SHORT), ((100, 129, 64), FWD),          # 128 / 129 keys
    ((65, 511, 32), FWD), ((65, 512, 32), KEYSPLIT), ((64, 512, 32), FWD), ((65, 512, 64), FWD),            # 512 keys, 65 queries, d = 32
    ((113, 530, 32, True), FWD), ((113, 532, 32, True), KEYSPLIT), ((113, 530, 32, False), KEYSPLIT),       # a mask needs Lk % 4 == 0
    ((1024, 1024, 64, True), FWD), ((1023, 1024, 64), FWD), ((1024, 1023, 64), FWD),                        # split-f16: no mask, >= 1024
    ((100, 100, 32, True, True), SHORT),
])
def test_dispatch_thresholds(args, kernel):
    assert plan(*args).kernel == kernel


def test_split_f16_rule_follows_the_switch():
    from dvis_plus_amd import functions as Fn
    want = X3 if Fn.x3_on() else FWD
    p = plan(1024, 1024, 64)
    assert p.kernel == want
    if want == X3:
        assert (p.nsplit, p.keys_per_split, p.qchunks) == (1, 1024, 8)
    with Fn.x3_disabled():
        assert plan(1024, 1024, 64).kernel == FWD


def test_plan_does_not_depend_on_the_batch():
    for args in [(100, 920, 32, True), (100, 333, 32, True), (130, 257, 64), (100, 100, 64)]:
        assert len({plan(*args, B=b) for b in (1, 2, 30)}) == 1


def test_splits_tile_the_keys():
    for args in [(200, 1035, 32, True), (113, 1025, 32), (100, 14720, 32, True), (1, 129, 64), (129, 511, 32), (17, 113, 32)]:
        p = plan(*args)
        Lq, Lk = args[:2]
        last = Lk - (p.nsplit - 1) * p.keys_per_split
        assert 0 < last <= p.keys_per_split, p
        assert p.qchunks == -(-Lq // {FWD: 128, SHORT: 16, KEYSPLIT: 112}[p.kernel])
    assert plan(200, 1035, 32, True).keys_per_split % 64 == 0 and plan(113, 1025, 32).keys_per_split % 16 == 0


def test_plan_refuses_what_the_launch_refuses():
    from dvis_plus_amd import functions as Fn
    with pytest.raises(RuntimeError, match="128"):
        plan(10, 129, short=True)
    with pytest.raises(RuntimeError, match="32 or 64"):
        Fn.attention_plan(torch.empty(4, 2, 32), torch.empty(4, 2, 32), 2)


def test_backward_threads():
    from dvis_plus_amd import functions as Fn
    assert [Fn.attention_backward_threads(n) for n in (1, 64, 65, 128, 129, 256)] == [64, 64, 128, 128, 256, 256]
    with pytest.raises(RuntimeError, match="256"):
        Fn.attention_backward_threads(257)
