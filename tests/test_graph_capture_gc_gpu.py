"""graphs.GraphRunner keeps the cyclic garbage collector out of a hipGraph capture: a dead cycle that holds an older graph frees
device memory in its destructor, which a capturing stream does not allow."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_no_cyclic_collection_inside_a_capture_and_the_collector_comes_back():
    from dvis_plus_amd.graphs import GraphRunner
    seen = []

    def fn(x):
        seen.append((torch.cuda.is_current_stream_capturing(), gc.isenabled()))
        return x * 2.0 + 1.0

    x = torch.arange(8, dtype=torch.float32, device="cuda:0")
    assert gc.isenabled()
    run = GraphRunner(fn)
    out = run("k", x)
    assert torch.equal(out, x * 2.0 + 1.0)
    assert (True, False) in seen and (True, True) not in seen      # captured with the collector off
    assert (False, True) in seen                                   # the warm-up calls ran with it on
    assert gc.isenabled()
    assert torch.equal(run("k", x + 1.0), (x + 1.0) * 2.0 + 1.0) and len(seen) == 3      # a replay, no new capture
    gc.disable()
    try:
        GraphRunner(fn)("k2", x)
        assert not gc.isenabled()                                  # a caller's own setting is left as it was
    finally:
        gc.enable()
