"""Timing of K15, the motion gate of cv/stabilizer.py (csrc/k15_motion.hip, Context.motion_update).

    python tools/time_motion.py [--windows 7] [--json profiles/motion_time.json]

For 1, 16 and 256 synthetic 1080p frames, BGR and gray, all in one run:
  k15            Context.motion_update into preallocated outputs, the product's launch shape
  one_launch / two_pass   the two launch shapes of the kernel file through the cross-check library (svx_ctx_set_motion_shape)
  composed       what the library offered for the same result before K15: Context.gray (BGR only), Context.resize_linear per frame,
                 then torch: stack, absdiff in int16, compare, sum
  floor          bytes / 8 TB/s, bytes = the taps the launch shape reads (4 per small pixel and frame, times the channels; the
                 one-launch shape reads the taps of every frame but the last twice) + the small images written + prev_small read
Every figure is the median (min, max) over `windows` windows of HIP-event time per call (_timing.event_ms); a window repeats the call until
it holds tens of milliseconds of work at least; every shape is warmed up by 3 calls first.  The outputs of k15 and composed are compared before timing.
detector_update_wall_ms: host clock around MotionDetector.update(frame on the device) -> bool, per frame; the read-back of the
count makes it latency-bound, so it is reported, not judged.
Exit status 1 when k15 is not ahead of composed at 16 x 1080p BGR.  Needs a GPU; there is no CPU path."""
import itertools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd.cv.stabilizer import MotionDetector  # noqa: E402
from _timing import cli, emit, event_ms, floor_ms, wall_ms  # noqa: E402

H, W, DW, DH = 1080, 1920, 160, 120
ITERS = {"k15": {1: 2000, 16: 1000, 256: 100}, "composed": {1: 300, 16: 40, 256: 4}}


def composed(ctx, frames, prev, threshold):
    gray = ctx.gray(frames) if frames.dim() == 4 else frames
    small = torch.stack([ctx.resize_linear(g, (DW, DH)) for g in gray])
    before = torch.cat([prev[None], small[:-1]]).to(torch.int16)
    counts = ((small.to(torch.int16) - before).abs() > threshold).sum((1, 2), dtype=torch.int32)
    return small, counts


def floor(n, ch, recompute):
    taps = 4 * DW * DH * ch
    nbytes = taps * (n + (n - 1 if recompute else 0)) + n * DW * DH * (1 if recompute else 3) + DW * DH
    return nbytes, floor_ms(nbytes)


def main():
    args = cli(__doc__, 7)
    window_ms = lambda fn, iters: event_ms(fn, iters, args.windows, warmup=3)[:3]
    ctx = sva.default_context()
    xlib = sva._native.lib_xcheck()
    xc = sva.Context(ctx.device, library=xlib)
    gen = torch.Generator(device=ctx.device).manual_seed(1234)
    prev = torch.randint(0, 256, (DH, DW), dtype=torch.uint8, device=ctx.device, generator=gen)
    res = {"what": "HIP-event ms per call, median (min, max) over windows; 1080p frames -> 160x120; one run", "windows": args.windows, "cases": []}
    for ch in (3, 1):
        for n in (1, 16, 256):
            shape = (n, H, W, 3) if ch == 3 else (n, H, W)
            frames = torch.randint(0, 256, shape, dtype=torch.uint8, device=ctx.device, generator=gen)
            out = (torch.empty((n, DH, DW), dtype=torch.uint8, device=ctx.device), torch.empty((n,), dtype=torch.int32, device=ctx.device))
            ctx.motion_update(frames, prev, 30.0, (DW, DH), out=out)
            want = composed(ctx, frames, prev, 30.0)
            assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]), "k15 and the composed path disagree"
            case = {"frames": n, "channels": ch}
            it = ITERS["k15"][n]
            case["k15_ms"] = window_ms(lambda: ctx.motion_update(frames, prev, 30.0, (DW, DH), out=out), it)
            for shape_id, name in ((0, "one_launch_ms"), (1, "two_pass_ms")):
                xc._check(xlib.svx_ctx_set_motion_shape(xc._h, shape_id), "svx_ctx_set_motion_shape")
                case[name] = window_ms(lambda: xc.motion_update(frames, prev, 30.0, (DW, DH), out=out), it)
            case["composed_ms"] = window_ms(lambda: composed(ctx, frames, prev, 30.0), ITERS["composed"][n])
            case["k15_ms_again"] = window_ms(lambda: ctx.motion_update(frames, prev, 30.0, (DW, DH), out=out), it)
            case["floor_bytes"], case["floor_ms"] = floor(n, ch, recompute=True)
            case["two_pass_floor_bytes"], case["two_pass_floor_ms"] = floor(n, ch, recompute=False)
            k15 = min(case["k15_ms"][0], case["k15_ms_again"][0])
            case["composed_over_k15"] = case["composed_ms"][0] / k15
            case["k15_over_floor"] = k15 / case["floor_ms"]
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            del frames, out, want
    xc.close()

    frames = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, device=ctx.device, generator=gen)
    det = MotionDetector()
    turn = itertools.count()
    # sync=False: update ends in the read-back of the count, so the device is idle before and after every call
    walls = wall_ms(lambda: det.update(frames[next(turn) & 1]), runs=300, warmup=20, sync=False)
    res["detector_update_wall_ms"] = {"median": walls.median, "min": walls.min, "max": walls.max, "calls": len(walls.values)}
    gate = next(c for c in res["cases"] if c["frames"] == 16 and c["channels"] == 3)
    res["k15_ahead_of_composed_at_16x1080p_bgr"] = max(gate["k15_ms"][0], gate["k15_ms_again"][0]) < gate["composed_ms"][0]
    emit(res, args.json)
    sys.exit(0 if res["k15_ahead_of_composed_at_16x1080p_bgr"] else 1)


if __name__ == "__main__":
    main()
