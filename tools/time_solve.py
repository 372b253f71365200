"""Times K14 (csrc/k14_solve.hip, Context.solve_sudoku into preallocated outputs): HIP-event time of the launch for 256 and 4096 frames
of two inputs -- what FramePipeline(resolve=True, propagate=True) hands to the solver on synth.py's frames (propagated_digits and
propagate_valid), and the sparse set of tests/solve_ref.py (17..30 clues, half with one clue falsified) -- next to a device copy of the
same bytes, sv_solve_sudoku_batch_host on 16 threads with the D2H and H2D copies a caller with device tensors needs around it, and
FramePipeline(resolve=True, propagate=True) frames/s with solve off and on.  Medians of repeated runs after a warm-up, with the spread (_timing.event_ms, wall_ms, wall_fps).

    python tools/time_solve.py [--out profiles/NAME.json]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import solve_ref as sr  # noqa: E402
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd.pipeline import FramePipeline  # noqa: E402
from sudoku_vision_amd.synth import random_state_dict, synth_frames  # noqa: E402
from _timing import emit, wall_ms  # noqa: E402
from time_propagate import launch_ms, pipeline_fps, spread_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = sva.default_context()
    ctx.load_state_dict(random_state_dict(1234))
    H, W, n_pool, chunk, repeat = 1080, 1920, 256, 64, 8
    frames = synth_frames(n_pool, H, W, seed=0, device="cuda")[0].contiguous()
    first = FramePipeline(ctx, H, W, chunk=chunk, resolve=True, propagate=True).run(frames)
    inputs = {"pipeline": (first["propagated_digits"].cpu().numpy(), first["propagate_valid"].cpu().numpy().astype(np.uint8)),
              "sparse": (sr.sparse_set(), None)}
    res = {"kernel": [], "max_nodes": 4096, "note": "frames drawn with repetition from each input set"}
    for name, (grids, active) in inputs.items():
        for n in (256, 4096):
            pick = np.arange(n) % len(grids)
            hg, ha = np.ascontiguousarray(grids[pick]), None if active is None else np.ascontiguousarray(active[pick])
            dg, da = torch.from_numpy(hg).to(ctx.device), None if ha is None else torch.from_numpy(ha).to(ctx.device)
            outs = ctx.solve_sudoku(dg, da)                         # allocated once: the timed calls only launch the kernel
            k = launch_ms(lambda: ctx.solve_sudoku(dg, da, out=outs))
            og = torch.empty_like(dg)
            c = launch_ms(lambda: og.copy_(dg))
            pg, ps, pr, pn = (torch.empty(s, dtype=t).pin_memory() for s, t in (((n, 81), torch.uint8), ((n, 81), torch.uint8), ((n,), torch.int8), ((n,), torch.int32)))
            hs, hr, hn = (torch.empty_like(outs[key]) for key in ("solution", "result", "nodes"))

            def on_host():
                pg.copy_(dg)                                        # D2H, then the solver, then H2D of what the device path leaves in HBM
                r, s, m = sva.host.solve_sudoku_batch(pg.numpy(), active=ha, max_nodes=4096, threads=16)
                ps.copy_(torch.from_numpy(s.reshape(n, 81))), pr.copy_(torch.from_numpy(r)), pn.copy_(torch.from_numpy(m))
                hs.copy_(ps, non_blocking=True), hr.copy_(pr, non_blocking=True), hn.copy_(pn, non_blocking=True)
            h = spread_ms(wall_ms(on_host, runs=15, warmup=3))
            assert all(torch.equal(a, outs[key]) for a, key in ((hs, "solution"), (hr, "result"), (hn, "nodes")))
            result = outs["result"].cpu().numpy()
            res["kernel"].append({"input": name, "frames": n, "solve": k, "copy_of_input": c, "host_16_threads_with_copies": h, "input_bytes": dg.numel(),
                                  "results": {int(v): int((result == v).sum()) for v in np.unique(result)},
                                  "nodes_mean": float(outs["nodes"].float().mean()), "nodes_max": int(outs["nodes"].max())})
            print(res["kernel"][-1], flush=True)

    res["pipeline"] = {}
    for name, on in (("solve_off", False), ("solve_on", True), ("solve_off_again", False), ("solve_on_again", True)):
        fps = pipeline_fps(FramePipeline(ctx, H, W, chunk=chunk, resolve=True, propagate=True, solve=on), frames, repeat)
        res["pipeline"][name] = {"frames_per_s_median": fps.median, "min": fps.min, "max": fps.max, "runs": 5,
                                 "frames": n_pool * repeat, "chunk": chunk, "shape": [H, W], "resolve": True, "propagate": True}
        print(name, res["pipeline"][name], flush=True)
    emit(res, args.out)


if __name__ == "__main__":
    main()
