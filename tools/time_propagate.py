"""Times K10 (csrc/k10_propagate.hip, Context.propagate_constraints into preallocated outputs): HIP-event time of the launch for 256 and
4096 frames of which 0 %, 10 % and 100 % are inconsistent (frames of tests/constraint_ref.py's generator), next to a device copy of the
kernel's input (the cost of one pass over it), the plain-Python restatement's time per frame on one CPU core, and FramePipeline
frames/s with resolve=True and propagate off and on.  Medians of repeated runs after a warm-up, with the spread (_timing.event_ms, wall_ms, wall_fps).

    python tools/time_propagate.py [--out profiles/NAME.json]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import constraint_ref as cr  # noqa: E402
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd.pipeline import FramePipeline  # noqa: E402
from sudoku_vision_amd.synth import random_state_dict, synth_frames  # noqa: E402
from _timing import emit, event_ms, wall_fps, wall_ms  # noqa: E402


def spread_ms(t):
    """A _timing.Timing under the keys the K9 / K10 / K14 records use."""
    return {"median_ms": t.median, "min_ms": t.min, "max_ms": t.max, "runs": len(t.values)}


def launch_ms(fn):
    """30 single launches after 5 warm-up calls."""
    return spread_ms(event_ms(fn, iters=1, windows=30, warmup=5))


def pipeline_fps(p, frames, repeat):
    """5 runs of `repeat` passes over the frames after one pass -> the Timing of frames/s."""
    p.run(frames)
    return wall_fps(lambda: p.run(frames, repeat=repeat), frames.shape[0] * repeat, runs=5, warmup=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = sva.default_context()
    digits, conf = cr.frames()
    good, bad = np.arange(cr.PER_KIND), np.arange(cr.PER_KIND, digits.shape[0])
    res = {"kernel": [], "note": "frames drawn with repetition from the 512 generated frames; inconsistent frames (the three misread kinds) "
                                 "spread evenly through the batch"}
    for n in (256, 4096):
        for share in (0.0, 0.1, 1.0):
            pick = good[np.arange(n) % good.size].copy()
            where = np.nonzero((np.arange(n) * share).astype(int) != ((np.arange(n) + 1) * share).astype(int))[0] if share < 1 else np.arange(n)
            pick[where] = bad[np.arange(where.size) % bad.size]
            dd, dc = torch.from_numpy(digits[pick]).to(ctx.device), torch.from_numpy(conf[pick]).to(ctx.device)
            od, oc = torch.empty_like(dd), torch.empty_like(dc)
            outs = ctx.propagate_constraints(dd, dc)                # allocated once: the timed calls only launch the kernel
            k = launch_ms(lambda: ctx.propagate_constraints(dd, dc, out=outs))
            c = launch_ms(lambda: (od.copy_(dd), oc.copy_(dc)))
            nbytes = dd.numel() + 4 * dc.numel()
            res["kernel"].append({"frames": n, "inconsistent_share": share, "inconsistent": int(where.size), "propagate": k, "copy_of_input": c,
                                  "input_bytes": nbytes, "iterations_mean": float(outs["iterations"].float().mean())})
            print(res["kernel"][-1], flush=True)
    for name, rows in (("consistent", good[:32]), ("inconsistent", bad[::12])):
        t = wall_ms(lambda: cr.propagate(digits[rows], conf[rows]), runs=3, warmup=0, sync=False)
        res[f"restatement_ms_per_{name}_frame_one_core"] = {"median": t.median / rows.size, "min": t.min / rows.size, "max": t.max / rows.size}
        print(name, res[f"restatement_ms_per_{name}_frame_one_core"], flush=True)

    ctx.load_state_dict(random_state_dict(1234))
    H, W, n, chunk, repeat = 1080, 1920, 256, 64, 8
    frames = synth_frames(n, H, W, seed=0, device="cuda")[0].contiguous()
    res["pipeline"] = {}
    for name, on in (("propagate_off", False), ("propagate_on", True), ("propagate_off_again", False), ("propagate_on_again", True)):
        fps = pipeline_fps(FramePipeline(ctx, H, W, chunk=chunk, resolve=True, propagate=on), frames, repeat)
        res["pipeline"][name] = {"frames_per_s_median": fps.median, "min": fps.min, "max": fps.max, "runs": 5,
                                 "frames": n * repeat, "chunk": chunk, "shape": [H, W], "resolve": True}
        print(name, res["pipeline"][name], flush=True)
    emit(res, args.out)


if __name__ == "__main__":
    main()
