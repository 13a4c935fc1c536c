"""ops.SideChain, the model forwards' one fork / join helper: one fork at construction, any number of `with chain:` blocks on the side stream, one join that
hands the blocks' results over to the forking stream.  The sequence below -- fork, two side blocks, join, a consumer on the forking stream -- is the shape of
_TriModel's forward (the answer GRU, later the batched v projection, behind ONE fork and ONE join).  All values are small integers: every result is exact."""
import pytest
import torch

from cti_amd import ops


def _run(x, side):
    """3 x + 1 as y = 2 x and z = y + 1 in two separate blocks of one chain, then w = z + x on the forking stream."""
    chain = ops.SideChain(side)
    with chain:
        y = 2 * x
    with chain:                                   # entered a second time: still behind the one fork, in launch order behind y
        z = y + 1
    chain.join(y, z)
    return z + x


def test_without_a_side_stream_everything_runs_in_place(monkeypatch):
    def untouched(*a, **k):
        raise AssertionError("SideChain(None) must not touch torch.cuda")
    for name in ("current_stream", "set_stream", "stream", "is_current_stream_capturing"):
        monkeypatch.setattr(torch.cuda, name, untouched)
    order = []
    chain = ops.SideChain(None)
    with chain as c:
        assert c is chain
        order.append("first")
    order.append("between")
    with chain:
        order.append("second")
    assert chain.join(torch.zeros(2), [None, (torch.ones(1),)], None) is None
    assert order == ["first", "between", "second"]
    x = torch.arange(64, dtype=torch.float32)
    assert torch.equal(_run(x, None), 3 * x + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [True, False])
def test_eager_fork_two_side_blocks_join(overlap):
    old = ops.use_aux_stream
    ops.use_aux_stream = overlap
    try:
        side = ops.aux_stream_object(torch.device("cuda", torch.cuda.current_device()))
        assert (side is not None) == overlap
        x = torch.arange(64, dtype=torch.float32, device="cuda")
        w = _run(x, side)
        torch.cuda.synchronize()
    finally:
        ops.use_aux_stream = old
    assert torch.equal(w.cpu(), 3 * torch.arange(64, dtype=torch.float32) + 1)


@pytest.mark.gpu
def test_captured_fork_two_side_blocks_join_replays_on_new_contents():
    dev = torch.device("cuda", torch.cuda.current_device())
    side = ops.aux_stream_object(dev)
    assert side is not None
    x = torch.arange(64, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        _run(x, side)                             # one eager warm-up on the capture stream
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            w = _run(x, side)
    torch.cuda.current_stream(dev).wait_stream(s)
    for contents in (torch.arange(64, dtype=torch.float32) * 5 - 7, torch.full((64,), 11.0)):
        x.copy_(contents)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(w.cpu(), 3 * contents + 1)
