"""Quality-gate timing (csrc/k6_quality.hip, FramePipeline(quality=True)) on 256 synthetic 1080p frames.

    python tools/time_quality.py [--frames 256] [--iters 50] [--steps 20] [--json out.json] [--kernels-only]

k_frame_quality_stats: HIP-event time per call (_timing.event_ms, one window of `iters` calls after one warm-up call), bytes = the BGR frames read once, against the 8 TB/s HBM peak.
k_grid_line_coverage (bits variant, as FramePipeline runs it): time per call; it reads a few of the bands' source words only.
FramePipeline: frames/s with quality off and on, alternated twice in this process (the same frames, chunk and host threads).
Needs a GPU; there is no CPU path."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd.pipeline import FramePipeline, host_cpu_budget  # noqa: E402
from sudoku_vision_amd.synth import synth_frames, random_state_dict  # noqa: E402
import _timing  # noqa: E402


def main():
    args = _timing.cli(__doc__, None, [
        ("--frames", dict(type=int, default=256)), ("--iters", dict(type=int, default=50)),
        ("--steps", dict(type=int, default=20, help="pipeline: passes over the pool per timed region")),
        ("--kernels-only", dict(action="store_true", help="skip the FramePipeline comparison (counter runs)"))])
    event_ms = lambda fn, iters: _timing.event_ms(fn, iters, windows=1, warmup=1).median
    n, H, W = args.frames, 1080, 1920
    ctx = sva.default_context()
    ctx.load_state_dict(random_state_dict(1234))
    frames, corners, _ = synth_frames(n, H, W, seed=1234, device="cuda")
    res = {"frames": n, "H": H, "W": W}

    outs = ctx.frame_quality_stats(frames)
    ms = event_ms(lambda: ctx.frame_quality_stats(frames, out=outs), args.iters)
    nbytes = n * H * W * 3
    res["stats"] = {"ms": ms, "bytes": nbytes, "GB_per_s": nbytes / ms / 1e6, "fraction_of_8TBps": nbytes / (ms * 1e-3) / _timing.HBM_PEAK_BYTES_PER_S,
                    "target_ms": 0.40}

    bits = ctx.preprocess_bits(frames)
    minv, ok = sva.Context.corners_to_minv_batch(corners, 450)
    md = ctx.minv_to_device(minv)
    cnt = ctx.grid_line_coverage(bits, md)
    ms = event_ms(lambda: ctx.grid_line_coverage(bits, md, out=cnt), args.iters)
    res["coverage_bits"] = {"ms": ms, "warped_px": n * 41400, "Gpx_per_s": n * 41400 / ms / 1e6, "target_ms": 0.05}
    binary = ctx.preprocess(frames)
    res["coverage_u8"] = {"ms": event_ms(lambda: ctx.grid_line_coverage(binary, md, out=cnt), args.iters)}
    del binary
    if args.kernels_only:
        _timing.emit(res, None)
        return

    host_threads = max(1, min(16, host_cpu_budget()) - 2)
    pipes = {q: FramePipeline(ctx, H, W, chunk=n, host_threads=host_threads, quality=q) for q in (False, True)}
    out = {"logits": torch.empty((n, 81, 10), dtype=torch.float32, device=ctx.device),
           "digits": torch.empty((n, 81), dtype=torch.uint8, device=ctx.device),
           "conf": torch.empty((n, 81), dtype=torch.float32, device=ctx.device)}
    for q in (False, True):
        pipes[q].run(frames, out=out, total=4 * n)
    rates = {False: [], True: []}
    for _ in range(2):
        for q in (False, True):
            pipes[q].run(frames, out=out, total=n)
            rates[q].append(_timing.wall_fps(lambda: pipes[q].run(frames, out=out, total=args.steps * n), args.steps * n, runs=1, warmup=0).median)
    off, on = max(rates[False]), max(rates[True])
    res["pipeline"] = {"frames_per_s_quality_off": rates[False], "frames_per_s_quality_on": rates[True], "ratio_best": on / off,
                       "target_ratio": 0.75, "host_threads": host_threads, "note": pipes[True].describe()}
    _timing.emit(res, args.json)


if __name__ == "__main__":
    main()
