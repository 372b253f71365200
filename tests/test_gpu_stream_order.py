"""GPU (-m gpu): every device entry of Context on a busy side stream and under graph replay (the case table: tests/stream_cases.py).

include/sudoku_vision_hip.h promises that every [dev] call is asynchronous on the stream it is given and that nothing synchronises the
device.  On the default stream with a synchronisation behind every call a launch, memset or copy that goes to another stream cannot be
seen; here it can.

Part 1 (every case): the input buffers hold A.  On a side stream s, with no synchronisation in between, a delay is enqueued, B is copied
into the buffers behind it, and the entry is called.  The result must be want(B): whatever part of the entry does not run on s, behind
the copy, reads A (or a half-reset counter) and is seen.  The imdecode family takes host bytes, so its hazard is the staging ring: three
decodes A, B, A (B's records outgrow A's set) queue behind one delay on a context of their own.
Part 2 (three controls, once, before Part 1): the same set-up with the entry called on the default stream instead.  It must see A: that
shows the delay is long enough for Part 1 to be able to fail.  Part 1 is skipped as measuring nothing when a control sees B.
Part 3 (every stream-pure case): the call is captured once into a graph on s (capture_error_mode "global": a launch on another stream, an
allocation by the library or a synchronisation raises) and replayed on B, on A, and on A again with nothing changed, which shows that
counters, job lists and accumulated outputs are reset by work inside the graph.

The delay is torch.cuda._sleep on s, calibrated once with two events; its length D is 200 times the median host time to issue one
warmed-up call.  Both are printed with the prefix STREAM; D is a property of this test, not a performance number."""
import statistics
import time

import numpy as np
import pytest
import torch

import stream_cases as sc

pytestmark = pytest.mark.gpu

D_FACTOR, D_LIMIT_MS = 200, 100.0


def _host(out):
    """a call's result, after a synchronisation -> tuple of numpy arrays and bytes"""
    return tuple(t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in out)


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, bytes) or isinstance(g, bytes):
            assert g == w, f"{what}: output {k} differs ({len(g)} and {len(w)} bytes)"
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what}: output {k} differs in {len(bad)} of {g.size} elements, first at {bad[0].tolist()}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}")


class Env:
    """The module's context, side stream, delay, and every case's buffers and expected results, made once."""

    def __init__(self):
        import sudoku_vision_amd as sva
        self.sva = sva
        self.ctx = sva.Context()
        sc.load_weights(self.ctx)
        self.xctx = None
        self.s = torch.cuda.Stream()
        self.prepared = {}
        self.cycles_per_ms = self._calibrate()
        self.issue_us = {}
        for case in sc.CASES:
            if case.kind == "pure":
                self.prepare(case)
        med = statistics.median(self.issue_us.values())
        self.delay_ms = D_FACTOR * med / 1000.0
        slowest = max(self.issue_us, key=self.issue_us.get)
        print(f"\nSTREAM issue time of one warmed-up call over {len(self.issue_us)} cases: median {med:.1f} us, "
              f"min {min(self.issue_us.values()):.1f} us, max {self.issue_us[slowest]:.1f} us ({slowest})")
        print(f"STREAM calibration: {self.cycles_per_ms:.0f} cycles of torch.cuda._sleep per ms")
        print(f"STREAM D = {D_FACTOR} x median = {self.delay_ms:.2f} ms")
        assert self.delay_ms <= D_LIMIT_MS, f"D = {self.delay_ms:.1f} ms is above {D_LIMIT_MS} ms: report it, do not use it"
        self.control_error = None

    def context(self, case):
        if not case.xcheck:
            return self.ctx
        if self.xctx is None:
            self.xctx = self.sva.Context(library=self.sva._native.lib_xcheck())
        return self.xctx

    def _calibrate(self):
        cycles = 20_000_000
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.s):
            torch.cuda._sleep(1000)                                # the first launch loads the kernel
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
        self.s.synchronize()
        return cycles / a.elapsed_time(b)

    def delay(self):
        """D of device work on the current stream"""
        torch.cuda._sleep(int(self.delay_ms * self.cycles_per_ms))

    def prepare(self, case):
        """Uploads A and B, warms the entry up on s, measures one un-synchronised issue, and computes want(A), want(B)."""
        if case.name in self.prepared:
            return self.prepared[case.name]
        ctx = self.context(case)
        A, B = case.inputs()
        dev = lambda inp: {k: (torch.from_numpy(v).to(ctx.device) if not k.startswith("_") else v) for k, v in inp.items()}
        A_dev, B_dev = dev(A), dev(B)
        buf = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in A_dev.items()}
        torch.cuda.synchronize()
        with torch.cuda.stream(self.s):
            case.call(ctx, buf)                                    # warm-up at this shape: code objects, scratch, torch's blocks
            self.s.synchronize()
            if case.kind == "pure":
                t0 = time.perf_counter()
                case.call(ctx, buf)
                self.issue_us[case.name] = (time.perf_counter() - t0) * 1e6
        torch.cuda.synchronize()
        if case.want is not None:
            want = (case.want(A), case.want(B))
        else:                                                      # eager, on the default stream, synchronised
            want = []
            for src in (A_dev, B_dev, A_dev):
                self.fill(buf, src)
                torch.cuda.synchronize()
                out = case.call(ctx, buf)
                torch.cuda.synchronize()
                want.append(_host(out))
            assert all(np.array_equal(x, y) for x, y in zip(want[0], want[2])), "the eager call does not repeat itself"
            assert any(not np.array_equal(x, y) for x, y in zip(want[0], want[1])), "the eager results for A and B are equal"
        p = self.prepared[case.name] = {"A": A, "B": B, "A_dev": A_dev, "B_dev": B_dev, "buf": buf, "want": {"A": want[0], "B": want[1]}}
        return p

    @staticmethod
    def fill(buf, src):
        for k, t in buf.items():
            if isinstance(t, torch.Tensor):
                t.copy_(src[k], non_blocking=True)

    def result(self, case, out, which, p):
        got = _host(out)
        return case.norm(got, p[which]) if case.norm else got


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_error():
    """A HIP error leaves the device in no state to go on with: nothing more is started on it in this run."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as err:
        pytest.exit(f"the GPU reported an error, stopping: {err}", 3)


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    if e.xctx is not None:
        e.xctx.close()


@pytest.fixture(scope="module")
def controls(env):
    """Part 2, once: each control entry on the default stream while the copy of B is held back on s.  -> None, or what went wrong."""
    for name in sc.CONTROLS:
        case = sc.by_name(name)
        p = env.prepare(case)
        env.fill(p["buf"], p["A_dev"])
        torch.cuda.synchronize()
        with torch.cuda.stream(env.s):
            env.delay()
            env.fill(p["buf"], p["B_dev"])
        out = case.call(env.ctx, p["buf"])                          # the default stream: not ordered with s
        torch.cuda.current_stream().synchronize()
        held = not env.s.query()
        got = env.result(case, out, "A", p)
        torch.cuda.synchronize()
        try:
            _same(got, p["want"]["A"], name)
        except AssertionError as err:
            try:
                _same(got, p["want"]["B"], name)
                return f"control {name} saw B: D = {env.delay_ms:.2f} ms is too short, Part 1 measures nothing"
            except AssertionError:
                return f"control {name} saw neither A nor B: {err}"
        print(f"STREAM control {name}: saw A; the delay was {'still' if held else 'no longer'} running when the entry had finished")
    return None


def test_controls_on_the_default_stream_see_a(controls):
    assert controls is None, controls


def _part1_buffers(env, case):
    ctx = env.context(case)
    p = env.prepare(case)
    env.fill(p["buf"], p["A_dev"])
    torch.cuda.synchronize()
    with torch.cuda.stream(env.s):
        env.delay()
        env.fill(p["buf"], p["B_dev"])
        out = case.call(ctx, p["buf"])
    env.s.synchronize()
    got = env.result(case, out, "B", p)
    torch.cuda.synchronize()
    _same(got, p["want"]["B"], f"{case.name} behind a late copy of B")


def _part1_decode(env, case):
    """Three decodes A, B, A behind one delay, on a context whose staging sets are its own: the second outgrows its set, which is
    regrown behind queued work.  The third refills the first one's set with the same bytes, so it cannot show a refill that came early."""
    A, B = case.inputs()
    want = {"A": case.want(A), "B": case.want(B)}
    ctx = env.sva.Context()
    try:
        with torch.cuda.stream(env.s):
            case.call(ctx, A)
            env.s.synchronize()
            env.delay()
            outs = [case.call(ctx, data) for data in (A, B, A)]
        env.s.synchronize()
        for k, (out, which) in enumerate(zip(outs, "ABA")):
            _same(_host(out), want[which], f"{case.name}: decode {k} (file {which}) of three behind one delay")
        torch.cuda.synchronize()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_input_written_late_on_a_side_stream(env, controls, name):
    if controls is not None:
        pytest.skip("a control of Part 2 failed: this case would measure nothing")
    case = sc.by_name(name)
    (_part1_decode if case.kind == "decode" else _part1_buffers)(env, case)


@pytest.mark.parametrize("name", sc.PURE)
def test_capture_once_replay_on_other_contents(env, name):
    """Part 3.  This is the test that found K6, K7's clahe and K19 zeroing their accumulators with hipMemsetAsync of 16 bytes or more,
    which a replayed graph carried out on its first replay only: frame_quality_stats passed replay 0 and gave lap_sum 139702862610904
    where 472 was due at replay 1.  They, and the 4n-byte counts of K15 and K7's pointwise tails (the _n5 cases: 20 bytes), now clear
    with a kernel of their own ("Stream order and graph replay")."""
    case = sc.by_name(name)
    ctx = env.context(case)
    p = env.prepare(case)
    env.fill(p["buf"], p["A_dev"])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, stream=env.s):
            out = case.call(ctx, p["buf"])
    except Exception:
        torch.cuda.synchronize()                                    # the context manager has ended the capture; nothing is tried again
        raise
    for step, which in enumerate(("B", "A", "A")):
        if step < 2:
            env.fill(p["buf"], p[which + "_dev"])
        g.replay()
        torch.cuda.synchronize()
        _same(env.result(case, out, which, p), p["want"][which], f"{case.name}: replay {step} on {which}")
    del g
