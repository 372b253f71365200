"""Timing of the cv/grid_v2.py drop-in (csrc/k13_grid_v2.hip, csrc/host_hough.cpp).

    python tools/time_grid_v2.py [--frames 16] [--iters 10] [--json profiles/grid_v2_time.json] [--parent-tree DIR]

Harris corners and the affine warp: HIP-event time inside the library (sv_timing_begin / sv_timing_end) on `frames` synthetic
1080p gray frames and on tests/golden/sample_4.jpg at full size, each beside the time a plain device copy of the same bytes
takes in the same run and beside bytes / 8 TB/s.  The Harris figure covers its four kernels (response, frame maximum,
candidates, sort + selection); one 1080p frame of uniform noise, where every local maximum is a candidate, shows what the
single-workgroup sort costs at its worst.  detect_grid: wall time of each of the four methods, called directly, on a 1080p synthetic
frame and on the photo (whichever method detect_grid itself would stop at).  --parent-tree DIR: a built checkout of the parent
commit; `python bench.py` is then run three times here and three times there after one unrecorded run of each, alternating, and both
headline values are recorded.
Needs a GPU; there is no CPU path."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd import imgcodecs  # noqa: E402
from sudoku_vision_amd.cv import grid_v2  # noqa: E402
from sudoku_vision_amd.synth import synth_frames  # noqa: E402
import _timing  # noqa: E402


def copy_ms(t, iters):
    dst = torch.empty_like(t)
    return _timing.event_ms(lambda: dst.copy_(t), iters, windows=1, warmup=1).median


def kernel_ms(ctx, name, fn, iters):
    fn()
    ctx.timing_begin()
    for _ in range(iters):
        fn()
    ms, launches = ctx.timing_end()[name]
    return ms / iters                                          # per call (a Harris call whose candidates overflow the default capacity runs twice)


def passes(ctx, gray, iters):
    """gray u8 [n,H,W] on the device -> the two kernel families' figures."""
    n, H, W = gray.shape
    nbytes = n * H * W
    floor = _timing.floor_ms(nbytes)
    copy = copy_ms(gray, iters)
    harris = kernel_ms(ctx, "k_harris", lambda: ctx.harris_corners(gray), iters)
    mats = np.stack([grid_v2._rotation_matrix((W // 2, H // 2), 7.0)] * n)
    md = torch.from_numpy(mats).to(ctx.device)
    warp = kernel_ms(ctx, "k_warp_affine", lambda: ctx.warp_affine(gray, md, (W, H), 255), iters)
    return {"frames": n, "H": H, "W": W, "bytes": nbytes, "copy_ms": copy, "bytes_over_8TBps_ms": floor,
            "harris_ms": harris, "harris_over_copy": harris / copy, "warp_affine_ms": warp, "warp_affine_over_copy": warp / copy}


def best_of_3_ms(fn):
    """fn's fastest of 3 runs, each from the same seed of the generator RANSAC draws from, and what it returned."""
    out, ms = [], []

    def keep():
        out[:] = [fn()]
    for _ in range(3):
        np.random.seed(0)
        ms.append(_timing.wall_ms(keep, runs=1, warmup=0).median)
    return min(ms), out[0]


def methods_ms(binary, gray):
    """Each method of detect_grid on its own (binary on the host, gray on the device) -> {method: wall ms, found}."""
    h, w = binary.shape

    def rotated():
        angle = grid_v2.detect_rotation_angle(binary)
        return grid_v2.detect_grid_contour(grid_v2.rotate_image(binary, angle if abs(angle) > 2 else 7.0)[0])

    def harris():
        corners = grid_v2.detect_corners_harris(gray)
        return grid_v2.fit_quadrilateral_ransac(corners, (h, w)) if len(corners) >= 4 else None

    out = {}
    for name, fn in (("contour", lambda: grid_v2.detect_grid_contour(binary)), ("lines", lambda: grid_v2.detect_grid_lines(binary)),
                     ("contour_rotated", rotated), ("harris_ransac", harris), ("detect_grid", lambda: grid_v2.detect_grid(binary, gray).method)):
        ms, res = best_of_3_ms(fn)
        out[name] = {"wall_ms": ms, "result": res if isinstance(res, str) else res is not None}
    return out


def bench_value(tree):
    out = subprocess.run([sys.executable, "bench.py"], cwd=tree, capture_output=True, text=True, check=True).stdout
    return json.loads(out.strip().splitlines()[-1])["value"]


def main():
    args = _timing.cli(__doc__, None, [("--frames", dict(type=int, default=16)), ("--iters", dict(type=int, default=10)),
                                       ("--parent-tree", dict(default=None, help="a built checkout of the parent commit, for the bench.py comparison"))])
    ctx = sva.default_context()
    frames, corners, _ = synth_frames(args.frames, 1080, 1920, seed=1234, device="cuda")
    gray = ctx.gray(frames)
    photo = imgcodecs.imread(os.path.join(ROOT, "tests", "golden", "sample_4.jpg"), device=True, ctx=ctx)
    photo_gray = ctx.gray(photo[None])
    res = {"synthetic_1080p": passes(ctx, gray, args.iters), "sample_4": passes(ctx, photo_gray, args.iters)}

    noise = torch.randint(0, 256, (1, 1080, 1920), dtype=torch.uint8, device=ctx.device)
    res["noise_1080p"] = passes(ctx, noise, max(2, args.iters // 5))

    res["detect_grid"] = {}
    for name, img in (("synthetic_1080p", frames[0]), ("sample_4", photo)):
        binary = ctx.preprocess(img[None].contiguous())[0].cpu().numpy()
        res["detect_grid"][name] = methods_ms(binary, ctx.gray(img[None].contiguous())[0])
    if args.parent_tree:
        trees = {"branch": ROOT, "parent": args.parent_tree}
        runs = {"branch": [], "parent": []}
        for tree in trees.values():                           # one unrecorded run each: the first bench of a session runs on a cold device
            bench_value(tree)
        for i in range(3):                                    # alternating, and the order within a pair alternates too
            for name in (("branch", "parent") if i % 2 == 0 else ("parent", "branch")):
                runs[name].append(bench_value(trees[name]))
        res["bench_headline_frames_per_s"] = runs
    _timing.emit(res, args.json)


if __name__ == "__main__":
    main()
