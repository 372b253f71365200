"""Times K24 (Context.dataset_cells, csrc/k24_dataset_cells.hip) at 810, 12,960 and 207,360 cells of 28 x 28 gray with Sub filters (what this
project's encoder and cv2 write), and on one batch of mixed geometry:
  - the launch alone (the packed bytes already on the device), HIP-event time,
next to
  - a device copy of the same bytes (filtered bytes in, u8 + f32 cells out),
  - those bytes / 8 TB/s,
  - the composed path on the same bytes: K19's gray read per geometry (Context.png_reconstruct(gray=True)), resize_linear per cell that is not
    28 x 28, preprocess_cells, torch's 255 - x and / 255,
  - the host half: sv_png_inflate_batch inside host.dataset_pack against zlib.decompress of the same IDAT streams on the same number of threads,
  - end to end on files in a temporary directory (12,960 at the most): ml/datasets.py's iterate_batches against Pillow's decode +
    tests/dataset_cells_ref.py on 16 threads, the latter timed on 810 files and scaled.  That is the numpy RESTATEMENT, not the reference:
    ml/datasets.py cannot run without cv2.
Medians over the windows with the spread (_timing.event_ms, wall_ms).  Speed is reported, not gated.  --smoke: 64 and 128 cells, one window.

    python tools/time_dataset_cells.py [--json profiles/dataset_cells_time.json] [--smoke]"""
import os
import sys
import tempfile
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "sudoku-vision_amd", "ml")]
import dataset_cells_ref as ref  # noqa: E402
import png_craft as craft  # noqa: E402
import png_decode_ref as decode_ref  # noqa: E402
import sudoku_vision_amd as sva  # noqa: E402
import datasets as ds  # noqa: E402
from _timing import cli, emit, event_ms, floor_ms, wall_ms  # noqa: E402

THREADS = 16
DISTINCT = 64
MIXED = [(28, 28, 0, 8), (50, 50, 0, 8), (64, 64, 6, 16), (29, 27, 0, 8), (33, 30, 2, 8), (9, 5, 0, 1), (64, 1, 0, 8), (40, 40, 4, 8)]   # W, H, type, depth


def stat(t):
    return {"median_ms": t.median, "min_ms": t.min, "max_ms": t.max}


def gray_files(k):
    return [craft.make_png(craft.random_samples(28, 28, 0, 8, seed=i), 0, 8, filters=1) for i in range(k)]


def mixed_files(k):
    out = []
    for i in range(k):
        w, h, t, d = MIXED[i % len(MIXED)]
        out.append(craft.make_png(craft.random_samples(h, w, t, d, seed=i), t, d, filters=[(r + i) % 5 for r in range(h)]))
    return out


def composed_path(ctx, files):
    """-> a callable that runs the composed path on device copies of the files' filtered bytes, and its number of launches per call"""
    infos, filtered, row_filters, status = sva.host.png_inflate_batch(files, threads=THREADS)
    assert not status.any()
    groups = {}
    for i, inf in enumerate(infos):
        groups.setdefault((inf.width, inf.height, inf.color_type, inf.bit_depth), []).append(i)
    dev = []
    for key, idx in groups.items():
        f = torch.from_numpy(np.stack([filtered[i] for i in idx])).to(ctx.device)
        r = torch.from_numpy(np.stack([row_filters[i] for i in idx])).to(ctx.device)
        dev.append((infos[idx[0]], f, r, key[:2] != (28, 28), idx, torch.tensor(idx, device=ctx.device)))
    n = len(files)
    cells = torch.empty((n, 28, 28), dtype=torch.uint8, device=ctx.device)

    def run():
        for info, f, r, resize, idx, where in dev:
            for a in range(0, f.shape[0], 65535):                    # K19 takes at most 65535 images a call
                gray, _ = ctx.png_reconstruct(info, f[a:a + 65535], r[a:a + 65535], gray=True)
                if resize:
                    for k in range(gray.shape[0]):
                        cells[idx[a + k]] = ctx.resize_linear(gray[k], (28, 28))
                elif len(dev) == 1:
                    cells[a:a + gray.shape[0]] = gray
                else:
                    cells[where[a:a + 65535]] = gray
        binary = ctx.preprocess_cells(cells)
        return (255 - binary).float().div_(255.0)
    return run


def device_row(ctx, files, repeat, res, label):
    packed = sva.host.dataset_pack(files, threads=THREADS)
    assert not packed.status.any()
    n = packed.n * repeat
    rec = np.tile(packed.records, repeat)                              # the same streams again: the bytes read per cell are what they are for n files
    dev = packed.pinned.to(ctx.device)
    filtered = dev[packed.filtered_at:packed.filtered_at + packed.filtered_size]
    records = torch.from_numpy(rec.view(np.uint8)).to(ctx.device)
    u8 = torch.empty((n, 28, 28), dtype=torch.uint8, device=ctx.device)
    f32 = torch.empty((n, 1, 28, 28), dtype=torch.float32, device=ctx.device)
    status = torch.empty(n, dtype=torch.int32, device=ctx.device)
    nbytes = packed.filtered_size * repeat + n * 784 * 5
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=ctx.device), torch.empty(nbytes, dtype=torch.uint8, device=ctx.device)
    k24 = lambda: ctx.dataset_cells_raw(filtered, records, None, sva._native.CELLS_DATASET, u8, f32, status)
    composed = composed_path(ctx, files * repeat)
    t = event_ms([k24, lambda: dst.copy_(src), composed], iters=res["iters"], windows=res["windows"], warmup=res["warmup"])
    assert torch.equal(composed().reshape(n, 1, 28, 28), f32), "the composed path and K24 differ"
    return {"cells": n, "batch": label, "bytes_in_and_out": nbytes, "k24_launch": stat(t[0]), "device_copy_of_the_same_bytes": stat(t[1]), "hbm_floor_ms": floor_ms(nbytes),
            "composed_k19_gray_resize_preprocess_torch": stat(t[2])}


def host_row(files, runs):
    infos = [sva.host.png_parse(f) for f in files]
    idats = [decode_ref.header(f)["idat"] for f in files]
    with ThreadPoolExecutor(THREADS) as pool:
        z = wall_ms(lambda: list(pool.map(zlib.decompress, idats, chunksize=max(1, len(idats) // (4 * THREADS)))), runs=runs, warmup=1, sync=False)
    ours = wall_ms(lambda: sva.host.png_inflate_batch(files, infos=infos, threads=THREADS), runs=runs, warmup=1, sync=False)
    pack = wall_ms(lambda: sva.host.dataset_pack(files, threads=THREADS), runs=runs, warmup=1, sync=False)
    return {"files": len(files), "threads": THREADS, "png_inflate_batch_wall": stat(ours), "zlib_decompress_same_threads_wall": stat(z), "dataset_pack_wall": stat(pack)}


def end_to_end_row(files, n_ref, runs):
    from PIL import Image
    with tempfile.TemporaryDirectory() as root:
        for i, f in enumerate(files):
            d = os.path.join(root, "train", str(i % 10))
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, f"{i}.png"), "wb") as fh:
                fh.write(f)
        data = ds.SyntheticDataset(root, "train")
        paths = [str(p) for p, _ in data.samples]

        def ours():
            for x, y in ds.iterate_batches(data, 4096, threads=THREADS):
                pass
            torch.cuda.synchronize()

        def one(path):
            return ref.cell_of_gray(np.asarray(Image.open(path).convert("L")))[1]

        with ThreadPoolExecutor(THREADS) as pool:
            cpu = wall_ms(lambda: list(pool.map(one, paths[:n_ref], chunksize=8)), runs=1, warmup=0, sync=False)
        t = wall_ms(ours, runs=runs, warmup=1)
    return {"files": len(files), "iterate_batches_wall": stat(t), "pillow_plus_dataset_cells_ref_16_threads_ms_scaled": cpu.median * len(files) / n_ref, "ref_files_timed": n_ref}


def main():
    args = cli(__doc__, 5, extra=[("--smoke", {"action": "store_true"})])
    ctx = sva.default_context()
    smoke = args.smoke
    res = {"rows": [], "iters": 2 if smoke else 20, "windows": 1 if smoke else args.windows, "warmup": 1 if smoke else 3}
    base = gray_files(DISTINCT)
    for n in ((64, 128) if smoke else (810, 12960, 207360)):
        files = (base * (min(n, 12960) // DISTINCT + 1))[:min(n, 12960)]
        res["rows"].append(device_row(ctx, files, n // len(files), res, "28x28 gray, Sub"))
        print(res["rows"][-1], flush=True)
    res["rows"].append(device_row(ctx, mixed_files(16 if smoke else 1072), 1, res, "mixed: " + ", ".join(f"{w}x{h} type {t} depth {d}" for w, h, t, d in MIXED)))
    print(res["rows"][-1], flush=True)
    files = (base * 203)[:128 if smoke else 12960]
    res["host"] = host_row(files, 1 if smoke else 3)
    res["end_to_end"] = end_to_end_row(files, 64 if smoke else 810, 1 if smoke else 3)
    res["note"] = ("the 207,360 row reads the 12,960 files' streams 16 times; the composed path's resize is one launch per cell that is not 28 x 28; the CPU column is "
                   "Pillow + tests/dataset_cells_ref.py, the numpy restatement, timed on 810 files and scaled, not the reference (which needs cv2)")
    emit(res, args.json)
    return res


if __name__ == "__main__":
    main()
