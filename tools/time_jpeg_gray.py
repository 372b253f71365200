"""Timing record of the grayscale JPEG read (csrc/host_jpeg.cpp's luma mode + csrc/k20_jpeg_gray.hip; Context.imdecode_batch(gray=True)) against
the colour read of the same files in the same build.

    python tools/time_jpeg_gray.py [--windows 5] [--threads 16] [--json profiles/jpeg_gray_time.json]

For 1 / 16 / 256 copies of one 1080p 4:2:0 quality-95 file (a 1080p crop of tests/golden/sample_1.jpg written by Pillow), at reduce 1, 2, 4, 8:
  gray_ms, colour_ms   HIP-event time per batch of the device half alone on records already in HBM, every image with records of its own:
                       sv_jpeg_reconstruct_sparse_gray_u8 (one launch) and sv_jpeg_reconstruct_sparse_bgr_u8 / _scaled_ (IDCT launches + the colour
                       kernel); *_dense_ms: the same through the dense int16 blocks
  copy_ms              a device-to-device copy of the gray output's bytes; floor_ms = (compact record bytes read + image bytes written) / 8 TB/s
  pcie_bytes           bytes per image that cross PCIe in imdecode_batch (compact transport), gray and colour
  e2e_fps              imdecode_batch + synchronize, frames per second, wall clock, `threads` host threads, gray and colour
  pillow_fps           Image.draft('L', ...) + np.asarray on a pool of `threads` threads, then one H2D copy of the frames
Medians over `windows` windows (_timing.event_ms, _timing.wall_fps); the first call of everything is a warm-up outside them."""
import ctypes as C
import io
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import jpeg_gray_ref as G  # noqa: E402
import png_encode_ref as R  # noqa: E402
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd import _native, host  # noqa: E402
import _timing  # noqa: E402

ITERS = {1: 20, 16: 5, 256: 1}


def staged(ctx, arrays, n):
    """n device copies of each host array (every image reads records of its own: 256 of them are past the Infinity Cache)"""
    return [torch.from_numpy(a.view(np.int16 if a.dtype.itemsize == 2 else np.int32 if a.dtype.itemsize == 4 else np.int64)).to(ctx.device)[None].repeat(n, 1)
            for a in arrays]


def main():
    args = _timing.cli(__doc__, 5, [("--threads", dict(type=int, default=16))])
    event_ms = lambda fn, iters: _timing.event_ms(fn, iters, args.windows, warmup=1).median
    wall_fps = lambda fn, n, windows=args.windows: _timing.wall_fps(fn, n, windows, warmup=1, sync=False).median  # the calls synchronise themselves
    from PIL import Image
    ctx = sva.default_context()
    lib = _native.lib()
    img = R.photo_1080p("sample_1.jpg")
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[:, :, ::-1]), "RGB").save(buf, "JPEG", quality=95, subsampling=2)
    data = buf.getvalue()
    stream = C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    ginfo, gm, go, gv, gq = host.jpeg_entropy_decode_luma_sparse(data)
    cinfo, cm, co, cv, cq = host.jpeg_entropy_decode_sparse(data)
    _, gcoef, _ = host.jpeg_entropy_decode_luma(data)
    _, ccoef, _ = host.jpeg_entropy_decode(data)
    gray_bytes = 12 * len(gm) + 2 * len(gv)
    colour_bytes = 12 * len(cm) + 2 * len(cv)
    result = {"threads": args.threads, "windows": args.windows, "file": "1080 x 1920, 4:2:0, quality 95, crop of tests/golden/sample_1.jpg",
              "file_bytes": len(data), "record_bytes": {"gray": gray_bytes, "colour": colour_bytes, "gray_dense": 2 * gcoef.size, "colour_dense": 2 * ccoef.size},
              "cases": []}
    pool = ThreadPoolExecutor(args.threads)
    dgq = torch.from_numpy(gq.view(np.int16)).to(ctx.device)
    dcq = torch.from_numpy(cq.view(np.int16).ravel()).to(ctx.device)
    for d in G.SCALES:
        h, w = -(-1080 // d), -(-1920 // d)
        want = G.pil_gray(data, d)
        for n in (1, 16, 256):
            case = {"reduce": d, "files": n}
            gray = torch.empty((n, h, w), dtype=torch.uint8, device=ctx.device)
            bgr = torch.empty((n, h, w, 3), dtype=torch.uint8, device=ctx.device)
            dm, do, dv = staged(ctx, (gm, go, gv), n)

            def run_gray():
                for i in range(n):
                    lib.sv_jpeg_reconstruct_sparse_gray_u8(ctx._h, C.byref(ginfo), p(dm[i]), p(do[i]), p(dv[i]), p(dgq), p(gray[i]), w, stream, d)
            case["gray_ms"] = event_ms(run_gray, ITERS[n])
            assert (gray[n - 1].cpu().numpy() == want).all()
            del dm, do, dv
            (dc,) = staged(ctx, (gcoef,), n)

            def run_gray_dense():
                for i in range(n):
                    lib.sv_jpeg_reconstruct_gray_u8(ctx._h, C.byref(ginfo), p(dc[i]), p(dgq), p(gray[i]), w, stream, d)
            case["gray_dense_ms"] = event_ms(run_gray_dense, ITERS[n])
            assert (gray[0].cpu().numpy() == want).all()
            del dc
            dm, do, dv = staged(ctx, (cm, co, cv), n)

            def run_colour():
                for i in range(n):
                    lib.sv_jpeg_reconstruct_sparse_scaled_bgr_u8(ctx._h, C.byref(cinfo), p(dm[i]), p(do[i]), p(dv[i]), p(dcq), p(bgr[i]), 3 * w, stream, d)
            case["colour_ms"] = event_ms(run_colour, ITERS[n])
            del dm, do, dv
            (dc,) = staged(ctx, (ccoef,), n)

            def run_colour_dense():
                for i in range(n):
                    lib.sv_jpeg_reconstruct_scaled_bgr_u8(ctx._h, C.byref(cinfo), p(dc[i]), p(dcq), p(bgr[i]), 3 * w, stream, d)
            case["colour_dense_ms"] = event_ms(run_colour_dense, ITERS[n])
            del dc
            dst = torch.empty_like(gray)
            case["copy_ms"] = event_ms(lambda: dst.copy_(gray), ITERS[n])
            case["floor_ms"] = _timing.floor_ms(n * (gray_bytes + h * w))
            del dst, bgr
            datas = [data] * n

            def e2e(is_gray):
                ctx.imdecode_batch(datas, threads=args.threads, reduce=d, gray=is_gray)
                torch.cuda.synchronize()
            case["e2e_fps"] = {"gray": wall_fps(lambda: e2e(True), n)}
            case["pcie_bytes"] = {"gray": ctx._jpeg_last_bytes}
            case["e2e_fps"]["colour"] = wall_fps(lambda: e2e(False), n)
            case["pcie_bytes"]["colour"] = ctx._jpeg_last_bytes
            m = min(n, 64)                                              # the host-only measurement: at most four rounds of the pool

            def pillow():
                frames = np.stack(list(pool.map(lambda x: G.pil_gray(x, d), datas[:m])))
                torch.from_numpy(frames).to(ctx.device)
                torch.cuda.synchronize()
            case["pillow_fps"] = wall_fps(pillow, m, max(1, args.windows // 2))
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
    _timing.emit(result, args.json)


if __name__ == "__main__":
    main()
