"""Timing record of the PNG decoder (csrc/host_png.cpp + csrc/k19_png_decode.hip; Context.imdecode_png_batch).

    python tools/time_png_decode.py [--windows 5] [--threads 16] [--json profiles/png_decode_time.json]

For 1 / 16 / 256 files of one 1080p BGR frame (a 1080p crop of tests/golden/sample_1.jpg), of three kinds -- `sub`: written by this project's
encoder with its defaults (every row Sub, every row a segment); `adaptive`: written by Pillow (its per-row choice); `paeth`: every row Paeth (one
segment of 1080 rows):
  device_ms        HIP-event time of the device half alone (Context.png_reconstruct: unfilter + expansion, three launches) on filtered bytes already
                   in HBM; copy_ms: a device-to-device copy of the same filtered bytes; floor_ms = (filtered + frame bytes) / 8 TB/s
  inflate_fps      the host half alone (host.png_inflate_batch) on `threads` threads, against zlib_fps: zlib.decompress of the same IDAT payloads
                   on a pool of `threads` threads
  e2e_fps          imdecode_png_batch + synchronize, frames per second, wall clock, `threads` host threads
  pillow_fps       Image.open(...).convert("RGB") on a pool of `threads` threads, then one H2D copy of the frames
Medians over `windows` windows (_timing.event_ms, _timing.wall_fps); the first call of everything is a warm-up outside them."""
import io
import json
import os
import sys
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import png_craft as K  # noqa: E402
import png_decode_ref as D  # noqa: E402
import png_encode_ref as R  # noqa: E402
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd import host  # noqa: E402
import _timing  # noqa: E402

ITERS = {1: 10, 16: 3, 256: 1}


def pillow_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    args = _timing.cli(__doc__, 5, [("--threads", dict(type=int, default=16))])
    event_ms = lambda fn, iters: _timing.event_ms(fn, iters, args.windows, warmup=1).median
    wall_fps = lambda fn, n, windows=args.windows: _timing.wall_fps(fn, n, windows, warmup=1, sync=False).median  # the calls synchronise themselves
    from PIL import Image
    ctx = sva.default_context()
    img = R.photo_1080p("sample_1.jpg")
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[:, :, ::-1]), "RGB").save(buf, "PNG")
    files = {"sub": ctx.imencode_png(torch.from_numpy(img).to(ctx.device)), "adaptive": buf.getvalue(),
             "paeth": K.make_png(img[:, :, ::-1].astype(np.int64), 2, 8, 4, level=1)}
    result = {"threads": args.threads, "windows": args.windows, "frame": "1080 x 1920 BGR, tests/golden/sample_1.jpg", "cases": []}
    pool = ThreadPoolExecutor(args.threads)
    for kind, data in files.items():
        assert (ctx.imdecode_png(data).cpu().numpy() == img).all(), kind
        info, filtered, row_filter = host.png_inflate(data)
        payload = D.header(data)["idat"]
        hist = np.bincount(row_filter, minlength=5).tolist()
        for n in (1, 16, 256):
            case = {"kind": kind, "files": n, "file_bytes": len(data), "filtered_bytes": int(info.filtered_bytes), "rows_per_filter": hist}
            f_dev = torch.from_numpy(filtered).to(ctx.device)[None].repeat(n, 1)
            r_dev = torch.from_numpy(row_filter).to(ctx.device)[None].repeat(n, 1)
            out = torch.empty((n, 1080, 1920, 3), dtype=torch.uint8, device=ctx.device)
            case["device_ms"] = event_ms(lambda: ctx.png_reconstruct(info, f_dev, r_dev, None, out), ITERS[n])
            assert (out[n - 1].cpu().numpy() == img).all()
            dst = torch.empty_like(f_dev)
            case["copy_ms"] = event_ms(lambda: dst.copy_(f_dev), ITERS[n])
            case["floor_ms"] = _timing.floor_ms(f_dev.numel() + out.numel())
            del f_dev, r_dev, dst
            datas = [data] * n
            m = min(n, 64)                                              # the host-only measurements: at most four rounds of the pool
            infos = [info] * m
            case["inflate_fps"] = wall_fps(lambda: host.png_inflate_batch(datas[:m], infos, threads=args.threads), m)
            case["zlib_fps"] = wall_fps(lambda: list(pool.map(zlib.decompress, [payload] * m)), m)

            def e2e():
                ctx.imdecode_png_batch(datas, threads=args.threads, out=out)
                torch.cuda.synchronize()
            case["e2e_fps"] = wall_fps(e2e, n)

            def pillow():
                frames = np.stack(list(pool.map(pillow_rgb, datas[:m])))
                torch.from_numpy(frames).to(ctx.device)
                torch.cuda.synchronize()
            case["pillow_fps"] = wall_fps(pillow, m, max(1, args.windows // 2))
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
    _timing.emit(result, args.json)


if __name__ == "__main__":
    main()
