"""tools/_timing.event_ms on the device: call counts, the shape of its record, and a side stream.  The timed call is a one-element add."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import _timing  # noqa: E402

pytestmark = pytest.mark.gpu


def counting_add(x, calls):
    def fn():
        calls.append(0)
        x.add_(1)
    return fn


def check(t, windows):
    assert len(t.values) == windows
    assert all(math.isfinite(v) and v > 0 for v in t.values)
    assert t.min <= t.median <= t.max
    assert t.min == min(t.values) and t.max == max(t.values)


def test_event_ms_one_callable(ctx):
    x, calls = torch.zeros(1, device=ctx.device), []
    t = _timing.event_ms(counting_add(x, calls), iters=4, windows=3, warmup=2)
    assert len(calls) == 2 + 12
    assert x.item() == 2 + 12
    check(t, 3)


def test_event_ms_sequence(ctx):
    x, calls = torch.zeros(1, device=ctx.device), ([], [])
    ts = _timing.event_ms([counting_add(x, calls[0]), counting_add(x, calls[1])], iters=4, windows=3, warmup=2)
    assert len(calls[0]) == len(calls[1]) == 2 + 12
    assert x.item() == 2 * (2 + 12)
    assert len(ts) == 2
    for t in ts:
        check(t, 3)


def test_event_ms_on_a_side_stream(ctx):
    """Work pending on another stream is neither waited for inside a window nor does it stop event_ms from returning."""
    side, other = torch.cuda.Stream(ctx.device), torch.cuda.Stream(ctx.device)
    x, y, calls = torch.zeros(1, device=ctx.device), torch.zeros(1 << 20, device=ctx.device), []
    side.wait_stream(torch.cuda.current_stream(ctx.device))
    other.wait_stream(torch.cuda.current_stream(ctx.device))
    with torch.cuda.stream(other):
        for _ in range(8):
            y.add_(1)
    with torch.cuda.stream(side):
        t = _timing.event_ms(counting_add(x, calls), iters=4, windows=3, warmup=2)
    assert len(calls) == 2 + 12
    check(t, 3)
    torch.cuda.synchronize(ctx.device)
    assert x.item() == 2 + 12 and y[0].item() == 8
