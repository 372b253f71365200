"""The measurement loops behind every timing record under profiles/: tools/time_*.py and tools/dev/*.py import them from here, and each passes
its own iters / windows / warmup, so two records are comparable once those three numbers are known.

  event_ms   HIP events on the current stream around `iters` calls, per window; ms per call
  wall_ms    time.perf_counter around `iters` calls, per run, with a device synchronise before the clock starts and before it stops; ms per call
  wall_fps   wall_ms turned into n / seconds
Each returns a Timing: median, min and max over the windows, and the windows' own values."""
import argparse
import json
import os
import statistics
import sys
import time
from typing import NamedTuple

HBM_PEAK_BYTES_PER_S = 8.0e12


class Timing(NamedTuple):
    """Statistics over the windows of one measurement; r[:3] is (median, min, max)."""
    median: float
    min: float
    max: float
    values: tuple


def _timing(values):
    return Timing(statistics.median(values), min(values), max(values), tuple(values))


def event_ms(fn, iters, windows, warmup):
    """HIP-event ms per call of fn on the current stream: `warmup` calls and a synchronise, then `windows` windows of record, `iters` calls,
    record, synchronise.  A sequence of callables gives a list of Timings, one per callable: each is warmed up in turn, and the windows
    alternate between them, so that what is compared sees the same clock and the same neighbours."""
    import torch
    fns = [fn] if callable(fn) else list(fn)
    for f in fns:
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    per_call = [[] for _ in fns]
    for _ in range(windows):
        for k, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            torch.cuda.synchronize()
            per_call[k].append(a.elapsed_time(b) / iters)
    out = [_timing(v) for v in per_call]
    return out[0] if callable(fn) else out


def wall_ms(fn, runs, warmup, sync=True, iters=1):
    """Host-clock ms per call of fn: `warmup` calls, then `runs` runs of `iters` calls.  sync: the device is synchronised before the clock
    starts and again before it stops, so a run holds the device work its calls enqueued and nothing else."""
    if sync:
        import torch
    for _ in range(warmup):
        fn()
    per_call = []
    for _ in range(runs):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        if sync:
            torch.cuda.synchronize()
        per_call.append((time.perf_counter() - t0) * 1e3 / iters)
    return _timing(per_call)


def wall_fps(fn, n, runs, warmup, sync=True, iters=1):
    """wall_ms of a call that handles n frames, as frames per second."""
    return _timing([n * 1e3 / ms for ms in wall_ms(fn, runs, warmup, sync, iters).values])


def floor_ms(nbytes):
    """The least time the HBM needs to move nbytes."""
    return nbytes / HBM_PEAK_BYTES_PER_S * 1e3


def cli(description, windows_default, extra=None):
    """The arguments every timing script takes (--windows unless windows_default is None, --json) plus its own, `extra` = [(flag, add_argument
    keywords)]; exits when there is no GPU."""
    ap = argparse.ArgumentParser(description=description, formatter_class=argparse.RawDescriptionHelpFormatter)
    if windows_default is not None:
        ap.add_argument("--windows", type=int, default=windows_default)
    ap.add_argument("--json", default=None)
    for flag, kw in extra or ():
        ap.add_argument(flag, **kw)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{os.path.basename(sys.argv[0])} needs a GPU")
    return args


def emit(result, json_path):
    """Prints the record and, given a path, writes it there."""
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if json_path:
        os.makedirs(os.path.dirname(os.path.abspath(json_path)), exist_ok=True)
        with open(json_path, "w") as fh:
            fh.write(text + "\n")
