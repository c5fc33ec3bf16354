"""policy/flat_learn.py's replay_learn_graph on a trivial step (8-element tensors): one capture
per key, replays that read the live inputs, None inputs, the cache emptied when the addresses
move, and a capture failure reported as None.  The failure is simulated on the host, as in the
policies' tests: the capture callable raises before any capture begins, so no stream is ever
left capturing."""
import warnings

import pytest
import torch

from tianshou_amd.policy.flat_learn import replay_learn_graph
from tianshou_amd.utils.capture import graph_capture

pytestmark = pytest.mark.gpu

N = 8


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _outputs(dev):
    return lambda: (torch.empty(N, device=dev), torch.empty((), device=dev))


def _step(static, out, total):
    x, w = static
    out.copy_(x * 2 + (w if w is not None else 0))
    total.copy_(out.sum())


class _Capture:
    """graph_capture, counting its calls."""

    def __init__(self):
        self.calls = 0

    def __call__(self, graph):
        self.calls += 1
        return graph_capture(graph)


def _rows(dev, seed):
    return torch.arange(N, dtype=torch.float32, device=dev) + seed


def test_capture_once_per_key_then_replay(dev):
    cache, capture = {}, _Capture()

    def run(key, addr, x, w):
        return replay_learn_graph(cache, key, addr, (x, w), _outputs(dev), _step, capture)

    x, w = _rows(dev, 0.0), _rows(dev, 100.0)
    total, out = run((N, True), ("a",), x, w)
    assert capture.calls == 1 and list(cache) == [(N, True)]
    assert torch.equal(out, x * 2 + w) and total.item() == (x * 2 + w).sum().item()
    st = cache[(N, True)]
    assert total is st["loss"] and out.data_ptr() != st["td"].data_ptr()
    assert [s.data_ptr() for s in st["static"]] != [x.data_ptr(), w.data_ptr()]

    # a replay reads the live inputs; the returned rows are a copy the next replay leaves alone
    x2, w2 = _rows(dev, 7.0), _rows(dev, -3.0)
    _, out2 = run((N, True), ("a",), x2, w2)
    assert capture.calls == 1 and len(cache) == 1
    assert torch.equal(out2, x2 * 2 + w2) and torch.equal(out, x * 2 + w)

    # a second key: a second entry, a None input stays None
    _, out3 = run((N, False), ("a",), x, None)
    assert capture.calls == 2 and set(cache) == {(N, True), (N, False)}
    assert cache[(N, False)]["static"][1] is None
    assert torch.equal(out3, x * 2)
    _, out4 = run((N, False), ("a",), x2, None)
    assert capture.calls == 2 and torch.equal(out4, x2 * 2)

    # the addresses moved: every graph of the cache goes before the new capture
    _, out5 = run((N, True), ("b",), x2, w)
    assert capture.calls == 3 and list(cache) == [(N, True)]
    assert cache[(N, True)]["addr"] == ("b",) and cache[(N, True)] is not st
    assert torch.equal(out5, x2 * 2 + w)


def test_capture_failure_is_reported(dev):
    cache, capture, tries = {}, _Capture(), []
    x, w = _rows(dev, 0.0), _rows(dev, 1.0)
    assert replay_learn_graph(cache, (N, True), ("a",), (x, w), _outputs(dev), _step,
                              capture) is not None

    def failing_capture(graph):
        tries.append(graph)
        raise RuntimeError("simulated capture failure")

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = replay_learn_graph(cache, (N, False), ("a",), (x, None), _outputs(dev), _step,
                                 failing_capture)
    assert out is None and len(tries) == 1
    msgs = [str(c.message) for c in caught if "learn-graph capture failed" in str(c.message)]
    assert len(msgs) == 1 and "simulated capture failure" in msgs[0]
    assert cache == {}
    assert not torch.cuda.is_current_stream_capturing()
