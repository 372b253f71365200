"""tools/_timing.py without a device: the host-clock loop calls what it is given as often as it says, and its record is ordered."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import _timing  # noqa: E402


def test_wall_ms_calls_fn_warmup_plus_runs_times():
    calls = []
    t = _timing.wall_ms(lambda: calls.append(sum(range(1000))), runs=7, warmup=3, sync=False)
    assert len(calls) == 3 + 7
    assert len(t.values) == 7
    assert 0 <= t.min <= t.median <= t.max
    assert t.min == min(t.values) and t.max == max(t.values)
    assert t[:3] == (t.median, t.min, t.max)


def test_wall_ms_iters_calls_per_run():
    calls = []
    t = _timing.wall_ms(lambda: calls.append(0), runs=4, warmup=1, sync=False, iters=5)
    assert len(calls) == 1 + 4 * 5
    assert len(t.values) == 4


def test_wall_fps_is_n_over_seconds():
    calls = []
    t = _timing.wall_fps(lambda: calls.append(sum(range(1000))), 16, runs=5, warmup=2, sync=False)
    assert len(calls) == 2 + 5
    assert len(t.values) == 5 and all(v > 0 for v in t.values)
    assert t.min <= t.median <= t.max


def test_floor_ms():
    assert _timing.HBM_PEAK_BYTES_PER_S == 8.0e12
    assert _timing.floor_ms(8e12) == 1000.0
    assert _timing.floor_ms(0) == 0.0


def test_emit_writes_what_it_prints(tmp_path, capsys):
    import json
    path = tmp_path / "sub" / "record.json"
    _timing.emit({"k15_ms": (1.0, 0.5, 2.0), "device_ms": 0.25}, str(path))
    want = {"k15_ms": [1.0, 0.5, 2.0], "device_ms": 0.25}
    assert json.loads(path.read_text()) == want
    assert json.loads(capsys.readouterr().out) == want
