"""Timing and size record of the PNG encoder (csrc/k18_png_encode.hip + csrc/host_png.cpp; Context.imencode_png_batch).

    python tools/time_png_encode.py [--windows 5] [--threads 16] [--json profiles/png_encode_time.json]
    python tools/time_png_encode.py --sizes [--json profiles/png_encode_size.json]

Timing, for 1 / 16 / 256 frames of 1080p BGR (a synthetic frame, and a 1080p crop of tests/golden/sample_1.jpg), default parameters (Sub, RLE):
  device_ms        HIP-event time of the device half alone (Context.png_deflate): filter, tokens, Huffman code, bit packing, compaction
  copy_ms          a device-to-device copy of the same frames, and floor_ms = bytes read / 8 TB/s
  pcie_bytes       compressed bytes + lengths that cross PCIe, against raw_bytes of the frames
  e2e_fps          imencode_png_batch frames per second, wall clock, with `threads` host threads
  zlib_fps         D2H copy of the raw frames, then zlib (level 1, Z_RLE) over the restatement's filter, one frame per thread of a pool of `threads`
  pillow_fps       the same with Pillow's writer, compress_level=1
--sizes: file size of one synthetic 1080p frame and the 1080p crops of sample_1.jpg and sample_4.jpg against len(zlib_rle(filtered)); the record
tests/test_gpu_png_encode.py asserts against (the ratio is deterministic)."""
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
import png_encode_ref as R  # noqa: E402
import sudoku_vision_amd as sva  # noqa: E402
import _timing  # noqa: E402

ITERS = {1: 20, 16: 5, 256: 1}


def sub_filter(img):
    rgb = np.ascontiguousarray(img[:, :, ::-1])
    f = np.empty((img.shape[0], 1 + 3 * img.shape[1]), np.uint8)
    f[:, 0] = 1
    flat = rgb.reshape(img.shape[0], -1)
    f[:, 1:4] = flat[:, :3]
    f[:, 4:] = flat[:, 3:] - flat[:, :-3]
    return f.tobytes()


def zlib_file(img):
    return R.make_file(img, R.zlib_rle(sub_filter(img)))


def pillow_file(img):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[:, :, ::-1]), "RGB").save(buf, "PNG", compress_level=1)
    return buf.getvalue()


def sizes(ctx):
    rec = {}
    for name in ("synthetic", "sample_1.jpg", "sample_4.jpg"):
        img = R.content("synthetic", 1080, 1920) if name == "synthetic" else R.photo_1080p(name)
        data = ctx.imencode_png(torch.from_numpy(img).to(ctx.device))
        assert (R.pillow_decode(data)[0] == img).all()
        ref = len(R.zlib_rle(R.filtered(img, "sub")))
        plan = ctx.png_encode_plan(1920, 1080, 3)
        rec[name] = {"file_bytes": len(data), "zlib_rle_bytes": ref, "ratio": len(data) / ref, "raw_bytes": int(img.size), "bands": int(plan.bands),
                     "band_rows": int(plan.band_rows)}
    return rec


def main():
    args = _timing.cli(__doc__, 5, [("--threads", dict(type=int, default=16)), ("--sizes", dict(action="store_true"))])
    event_ms = lambda fn, iters: _timing.event_ms(fn, iters, args.windows, warmup=1).median
    wall_fps = lambda fn, n, windows=args.windows: _timing.wall_fps(fn, n, windows, warmup=1, sync=False).median  # the calls end in a read-back
    ctx = sva.default_context()
    if args.sizes:
        result = sizes(ctx)
    else:
        result = {"threads": args.threads, "windows": args.windows, "cases": []}
        assert R.photo_1080p("sample_1.jpg").shape == (1080, 1920, 3)
        assert sub_filter(R.content("synthetic", 40, 64)) == R.filtered(R.content("synthetic", 40, 64), "sub")
        pool = ThreadPoolExecutor(args.threads)
        for name in ("synthetic", "sample_1.jpg"):
            img = R.content("synthetic", 1080, 1920) if name == "synthetic" else R.photo_1080p(name)
            plan = ctx.png_encode_plan(1920, 1080, 3)
            for n in (1, 16, 256):
                frames = torch.from_numpy(img).to(ctx.device)[None].repeat(n, 1, 1, 1)
                case = {"content": name, "frames": n, "raw_bytes": int(frames.numel())}
                case["device_ms"] = event_ms(lambda: ctx.png_deflate(frames, plan), ITERS[n])
                dst = torch.empty_like(frames)
                case["copy_ms"] = event_ms(lambda: dst.copy_(frames), ITERS[n])
                case["floor_ms"] = _timing.floor_ms(frames.numel())
                lens = ctx.png_deflate(frames, plan)[1]
                case["pcie_bytes"] = int(lens.sum().item()) + 12 * int(lens.numel())
                case["e2e_fps"] = wall_fps(lambda: ctx.imencode_png_batch(frames, threads=args.threads), n)
                m = min(n, 16)                                         # the host writers: at most one round of the pool

                def host(writer):
                    host_frames = frames[:m].cpu().numpy()
                    return list(pool.map(writer, host_frames))
                case["zlib_fps"] = wall_fps(lambda: host(zlib_file), m, max(1, args.windows // 2))
                case["pillow_fps"] = wall_fps(lambda: host(pillow_file), m, max(1, args.windows // 2))
                result["cases"].append(case)
                print(json.dumps(case), flush=True)
    _timing.emit(result, args.json)


if __name__ == "__main__":
    main()
