"""Times K9 (csrc/k9_resolve.hip, Context.resolve_conflicts into preallocated outputs): HIP-event time of the launch for 256 and 4096 frames of which 0 %, 10 %
and 100 % break the sudoku rules (frames of tests/resolve_ref.py's generator), next to a device copy of the same top-k arrays (the
cost of one pass over them), the plain-Python restatement's time per conflicted frame on one CPU core, and FramePipeline frames/s
with resolve off and on.  Medians of repeated runs after a warm-up, with the spread (_timing.event_ms, wall_ms, wall_fps).

    python tools/time_resolve.py [--out profiles/NAME.json]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import resolve_ref as rr  # noqa: E402
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd.pipeline import FramePipeline  # noqa: E402
from sudoku_vision_amd.synth import random_state_dict, synth_frames  # noqa: E402
from _timing import emit, wall_ms  # noqa: E402
from time_propagate import launch_ms, pipeline_fps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = sva.default_context()
    index, prob = rr.frames(77, 1024)
    ref = rr.resolve(index, prob)
    bad = np.nonzero(ref["num_conflicts_before"] > 0)[0]
    good = np.nonzero(ref["num_conflicts_before"] == 0)[0]
    res = {"kernel": [], "note": "frames drawn with repetition from 1024 generated frames; conflicted frames spread evenly through the batch"}
    for n in (256, 4096):
        for share in (0.0, 0.1, 1.0):
            pick = good[np.arange(n) % good.size].copy()
            where = np.nonzero((np.arange(n) * share).astype(int) != ((np.arange(n) + 1) * share).astype(int))[0] if share < 1 else np.arange(n)
            pick[where] = bad[np.arange(where.size) % bad.size]
            di, dp = torch.from_numpy(index[pick]).to(ctx.device), torch.from_numpy(prob[pick]).to(ctx.device)
            oi, op = torch.empty_like(di), torch.empty_like(dp)
            outs = ctx.resolve_conflicts(di, dp)                 # allocated once: the timed calls only launch the kernel
            k = launch_ms(lambda: ctx.resolve_conflicts(di, dp, out=outs))
            c = launch_ms(lambda: (oi.copy_(di), op.copy_(dp)))
            nbytes = di.numel() + 4 * dp.numel()
            res["kernel"].append({"frames": n, "conflicted_share": share, "conflicted": int(where.size), "resolve": k, "copy_of_topk": c,
                                  "topk_bytes": nbytes, "copy_GBps": 2 * nbytes / c["median_ms"] / 1e6})
            print(res["kernel"][-1], flush=True)
    sub = bad[:64]
    t = wall_ms(lambda: rr.resolve(index[sub], prob[sub]), runs=3, warmup=0, sync=False)
    res["restatement_ms_per_conflicted_frame_one_core"] = {"median": t.median / sub.size, "min": t.min / sub.size, "max": t.max / sub.size}
    print(res["restatement_ms_per_conflicted_frame_one_core"], flush=True)

    ctx.load_state_dict(random_state_dict(1234))
    H, W, n, chunk, repeat = 1080, 1920, 256, 64, 8
    frames = synth_frames(n, H, W, seed=0, device="cuda")[0].contiguous()
    res["pipeline"] = {}
    for name, on in (("resolve_off", False), ("resolve_on", True), ("resolve_off_again", False)):
        fps = pipeline_fps(FramePipeline(ctx, H, W, chunk=chunk, resolve=on), frames, repeat)
        res["pipeline"][name] = {"frames_per_s_median": fps.median, "min": fps.min, "max": fps.max, "runs": 5,
                                 "frames": n * repeat, "chunk": chunk, "shape": [H, W]}
        print(name, res["pipeline"][name], flush=True)
    emit(res, args.out)


if __name__ == "__main__":
    main()
