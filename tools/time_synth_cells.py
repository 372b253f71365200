"""Times K23 behind ml/generate_synthetic_v2.py's generate_batch at 810, 12,960 and 207,360 cells of 28 x 28, all ten classes in equal parts:
  - the launch alone (Context.synth_cells with the job already on the device), HIP-event time,
  - generate_batch whole: the host's job build (the draws from `random`, in Python), the upload and the launch, wall clock,
next to
  - a device copy of the output bytes,
  - those bytes / 8 TB/s,
  - tests/synth_cells_ref.py on the CPU for the same job, wall clock, run on the first 810 outputs and scaled to the row's count.  That is
    the numpy RESTATEMENT of the contract, not the reference: ml/generate_synthetic_v2.py cannot run without cv2.
The glyphs are a ring mask per digit (tests/test_synth_cells_ref.py's RingFont), so that the tool needs no font.  The job of the largest
row is the 12,960-cell job repeated 16 times: the draws are Python's and their build time is reported from the 12,960 row.
Medians over the windows with the spread (_timing.event_ms, wall_ms).  Speed is reported, not gated.

    python tools/time_synth_cells.py [--json profiles/synth_cells_time.json]"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "sudoku-vision_amd", "ml")]
import synth_cells_ref as sr  # noqa: E402
import test_synth_cells_ref as cpu_tests  # noqa: E402
import sudoku_vision_amd as sva  # noqa: E402
import generate_synthetic_v2 as gen  # noqa: E402
from _timing import cli, emit, event_ms, floor_ms, wall_ms  # noqa: E402

REF_OUTPUTS = 810


def stat(t):
    return {"median_ms": t.median, "min_ms": t.min, "max_ms": t.max}


def main():
    args = cli(__doc__, 5)
    ctx = sva.default_context()
    fonts = [("ring", cpu_tests.RingFont())]
    res = {"rows": [], "iters": 20, "windows": args.windows, "warmup": 3}
    job = None
    for n in (810, 12960, 207360):
        labels = [k % 10 for k in range(min(n, 12960))]
        random.seed(1)
        np.random.seed(1)
        if n <= 12960:
            job = gen.build_cells(labels, fonts, 28)
        cells, steps, n_steps, atlas = job
        rep = n // len(cells)
        cells, steps, n_steps = np.tile(cells, rep), np.tile(steps, (rep, 1)), np.tile(n_steps, rep)
        dev = ctx.synth_upload_program(cells, steps, n_steps, 28, atlas)
        out = torch.empty((n, 28, 28), dtype=torch.uint8, device=ctx.device)
        nbytes = n * 784
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device=ctx.device), torch.empty(nbytes, dtype=torch.uint8, device=ctx.device)
        launch, copy = event_ms([lambda: ctx.synth_cells(dev[0], dev[1], dev[2], 28, dev[3], seed=3, out=out), lambda: dst.copy_(src)], iters=res["iters"],
                                windows=args.windows, warmup=res["warmup"])
        row = {"outputs": n, "mean_steps": float(n_steps.mean()), "output_bytes": nbytes, "record_bytes_read": n * (96 + 960 + 4), "k23_launch": stat(launch),
               "device_copy_of_the_output_bytes": stat(copy), "hbm_floor_ms": floor_ms(nbytes)}
        if n <= 12960:
            row["generate_batch_wall"] = stat(wall_ms(lambda: gen.generate_batch(labels, fonts, 28, seed=3), runs=3, warmup=1))
            row["host_job_build_wall"] = stat(wall_ms(lambda: gen.build_cells(labels, fonts, 28), runs=3, warmup=1, sync=False))
        m = min(n, REF_OUTPUTS)
        ref = wall_ms(lambda: sr.run_job(cells[:m], steps[:m], n_steps[:m], 28, atlas, seed=3), runs=1, warmup=0, sync=False)
        row["synth_cells_ref_numpy_restatement_cpu_ms_scaled"] = ref.median * n / m
        row["synth_cells_ref_outputs_timed"] = m
        res["rows"].append(row)
        print(row, flush=True)
    res["note"] = ("the CPU column is tests/synth_cells_ref.py, the numpy restatement of the contract, timed on 810 outputs and scaled, not the reference (which "
                   "needs cv2); generate_batch's wall time is dominated by the host's job build, Python draws from `random` one cell at a time; the 207,360 row "
                   "repeats the 12,960-cell job 16 times")
    emit(res, args.json)


if __name__ == "__main__":
    main()
