"""Timing of K16, the solution overlay (csrc/k16_overlay.hip, Context.render_overlay).

    python tools/time_overlay.py [--windows 7] [--json profiles/overlay_time.json]

For 1, 16 and 256 synthetic 1080p frames, a small quad (140 px) and a large one (980 px), all in one run:
  in_place       Context.render_overlay(out=frames): the kernel alone; it touches only the blocks the grid reaches
  out_of_place   Context.render_overlay into a preallocated destination: a device copy of the frames, then the same kernel
  copy           dst.copy_(frames): the device copy of the same bytes (what out_of_place cannot be faster than)
  floor          bytes / 8 TB/s: in place, the pixels the reference changes, read and written (3 bytes each way); out of place, all frames
                 read and written
Every figure is the median (min, max) over `windows` windows of HIP-event time per call (_timing.event_ms); a window repeats the call until it holds tens
of milliseconds of work at least; every shape is warmed up first, and the in-place result of the first frame is compared with the
out-of-place one before timing.  Drawing in place again and again changes the pixel values, not the work.
stream_wall_ms: host clock per frame of pipeline.recognize_stream over 40 repeats of one synthetic 1080p frame, the recogniser handed a
solvable grid, with overlay off and on; the loop synchronises with the host every frame, so it is reported, not judged.
Needs a GPU; there is no CPU path."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd import pipeline  # noqa: E402
from sudoku_vision_amd.synth import random_state_dict, synth_frames  # noqa: E402
from _timing import cli, emit, event_ms, floor_ms  # noqa: E402

H, W = 1080, 1920
ITERS = {1: 2000, 16: 400, 256: 25}
QUADS = {"small_140px": np.array([[1203, 411], [1342, 420], [1335, 560], [1198, 548]], np.float32),
         "large_980px": np.array([[470, 52], [1452, 40], [1466, 1030], [455, 1018]], np.float32)}


def stream_wall_ms(ctx, frame, given, overlay, repeats=40):
    real = ctx.frames_to_digits
    logits = torch.full((1, 81, 10), -4.0, device=ctx.device)
    logits[0, torch.arange(81), torch.from_numpy(given.astype(np.int64))] = 6.0

    def reads_given(chunk, minv, out=None, **kw):                 # the recogniser as it is, then a solvable reading in place of its own
        r = real(chunk, minv, out=out, **kw)
        r["logits"].copy_(logits)
        r["digits"].copy_(logits.argmax(-1).to(torch.uint8))
        r["conf"].copy_(torch.softmax(logits, -1).max(-1).values)
        return r
    ctx.frames_to_digits = reads_given
    try:
        walls, solved = [], 0
        feed = pipeline.recognize_stream([frame] * repeats, ctx=ctx, glue=sva.Context.GLUE_NORMALIZE, overlay=overlay)
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = next(feed)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            solved += int(overlay and r["solve_result"] == 1)
        steady = walls[5:]
        return {"median": statistics.median(steady), "min": min(steady), "max": max(steady), "frames": len(steady), "frames_drawn": solved}
    finally:
        del ctx.frames_to_digits


def main():
    args = cli(__doc__, 7)
    window_ms = lambda fn, iters: event_ms(fn, iters, args.windows, warmup=3)[:3]
    ctx = sva.default_context()
    gen = torch.Generator(device=ctx.device).manual_seed(1234)
    rs = np.random.RandomState(1)
    res = {"what": "HIP-event ms per call, median (min, max) over windows; 1080p BGR frames; one run", "windows": args.windows, "cases": []}
    for n in (1, 16, 256):
        frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=ctx.device, generator=gen)
        work = torch.empty_like(frames)
        dst = torch.empty_like(frames)
        digits = torch.from_numpy(rs.randint(1, 10, (n, 81)).astype(np.uint8)).to(ctx.device)
        for name, quad in QUADS.items():
            m, ok = sva.Context.corners_to_m_batch(np.repeat(quad[None], n, 0))
            assert ok.all()
            m_dev = ctx.minv_to_device(m)
            ctx.render_overlay(frames, m_dev, digits, out=dst)
            work.copy_(frames)
            ctx.render_overlay(work, m_dev, digits, out=work)
            assert torch.equal(work, dst), "in place and out of place disagree"
            drawn = int((dst[0] != frames[0]).any(-1).sum().item())
            case = {"frames": n, "quad": name, "pixels_changed_in_frame_0": drawn}
            case["in_place_ms"] = window_ms(lambda: ctx.render_overlay(work, m_dev, digits, out=work), ITERS[n])
            case["out_of_place_ms"] = window_ms(lambda: ctx.render_overlay(frames, m_dev, digits, out=dst), ITERS[n])
            case["copy_ms"] = window_ms(lambda: dst.copy_(frames), ITERS[n])
            case["in_place_ms_again"] = window_ms(lambda: ctx.render_overlay(work, m_dev, digits, out=work), ITERS[n])
            case["in_place_floor_bytes"] = 6 * drawn * n
            case["in_place_floor_ms"] = floor_ms(case["in_place_floor_bytes"])
            case["out_of_place_floor_bytes"] = 2 * frames.numel()
            case["out_of_place_floor_ms"] = floor_ms(case["out_of_place_floor_bytes"])
            case["out_of_place_over_copy"] = case["out_of_place_ms"][0] / case["copy_ms"][0]
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
        del frames, work, dst

    frame = synth_frames(1, H, W, seed=11, device="cuda")[0][0]
    ctx.load_state_dict(random_state_dict(1234))
    r, c = np.divmod(np.arange(81), 9)
    given = ((3 * (r % 3) + r // 3 + c) % 9 + 1).astype(np.uint8)             # a valid solved grid, 45 cells blanked: solvable
    given[np.random.RandomState(2).choice(81, 45, replace=False)] = 0
    res["stream_wall_ms"] = {"overlay_off": stream_wall_ms(ctx, frame, given, False), "overlay_on": stream_wall_ms(ctx, frame, given, True)}
    emit(res, args.json)


if __name__ == "__main__":
    main()
