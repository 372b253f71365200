"""Times K22 behind ml/augment_data.py's augment_batch for the three presets at 81, 1296 and 20,736 cells of 28 x 28, multiplier 10:
  - the launch alone (Context.augment with the program already on the device), HIP-event time,
  - augment_batch whole: the host's program build (the draws from `random`, in Python), the upload and the launch, wall clock,
next to
  - a device copy of the bytes the launch reads and writes (images in, step records in, images out),
  - those bytes / 8 TB/s,
  - tests/augment_ref.py on the CPU for the same program (on at most 810 outputs, scaled), wall clock.  That is the numpy RESTATEMENT
    of the contract, not the reference: tools/augment_data.py cannot run without cv2.
Medians over the windows with the spread (_timing.event_ms, wall_ms).  Speed is reported, not gated.

    python tools/time_augment.py [--json profiles/augment_time.json]"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "sudoku-vision_amd", "ml")]
import augment_ref as ar  # noqa: E402
import sudoku_vision_amd as sva  # noqa: E402
import augment_data as aug  # noqa: E402
from _timing import cli, emit, event_ms, floor_ms, wall_ms  # noqa: E402

MULTIPLIER, REF_OUTPUTS = 10, 810


def stat(t):
    return {"median_ms": t.median, "min_ms": t.min, "max_ms": t.max}


def main():
    args = cli(__doc__, 5)
    ctx = sva.default_context()
    res = {"rows": [], "iters": 20, "windows": args.windows, "warmup": 3, "multiplier": MULTIPLIER}
    for n in (81, 1296, 20736):
        images_h = ar.sample_images(81, 28, 28, seed=1)[np.arange(n) % 81]
        images = torch.from_numpy(images_h).to(ctx.device)
        for preset in ("light", "medium", "heavy"):
            random.seed(1)
            np.random.seed(1)
            steps, n_steps, si = aug.build_program(n, 28, 28, MULTIPLIER, aug.create_augmentation_pipeline(preset), 3)
            dev = ctx.augment_upload_program(steps, n_steps, si, n, 28, 28)
            n_out = n * MULTIPLIER
            out = torch.empty((n_out, 28, 28), dtype=torch.uint8, device=ctx.device)
            nbytes = n * 784 + n_out * (784 + steps.dtype.itemsize * steps.shape[1] + 8)
            src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=ctx.device), torch.empty(nbytes // 2, dtype=torch.uint8, device=ctx.device)
            launch, copy = event_ms([lambda: ctx.augment(images, *dev, seed=3, out=out), lambda: dst.copy_(src)], iters=res["iters"], windows=args.windows,
                                    warmup=res["warmup"])
            whole = wall_ms(lambda: aug.augment_batch(images, MULTIPLIER, preset, 3, seed=3), runs=3, warmup=1)
            build = wall_ms(lambda: aug.build_program(n, 28, 28, MULTIPLIER, aug.create_augmentation_pipeline(preset), 3), runs=3, warmup=1, sync=False)
            m = min(n_out, REF_OUTPUTS)
            cpu = wall_ms(lambda: ar.run_program(images_h, steps[:m], n_steps[:m], si[:m], seed=3), runs=1, warmup=0, sync=False)
            row = {"cells": n, "outputs": n_out, "preset": preset, "mean_steps": float(n_steps.mean()), "bytes_read_and_written": nbytes, "k22_launch": stat(launch),
                   "device_copy_same_bytes": stat(copy), "hbm_floor_ms": floor_ms(nbytes), "augment_batch_wall": stat(whole), "host_program_build_wall": stat(build),
                   "augment_ref_numpy_restatement_cpu_ms_scaled": cpu.median * n_out / m, "augment_ref_outputs_timed": m}
            res["rows"].append(row)
            print(row, flush=True)
    res["note"] = ("the CPU column is tests/augment_ref.py, the numpy restatement of the contract, not the reference (which needs cv2); augment_batch's wall "
                   "time is dominated by the host's program build, Python draws from `random` one chain at a time")
    emit(res, args.json)


if __name__ == "__main__":
    main()
