"""Timing of the JPEG encoder (csrc/k17_jpeg_encode.hip + the Huffman packer of csrc/host_jpeg.cpp; Context.imencode_batch).

    python tools/time_jpeg_encode.py [--windows 5] [--threads 16] [--json profiles/jpeg_encode_time.json]

For 1, 16 and 256 1080p BGR frames, a synthetic frame with the solution drawn in (K16) and tests/golden/sample_1.jpg tiled to size, quality 75 and
95 at 4:2:0, all in one run:
  device_ms        HIP-event time of the device half alone (Context.jpeg_forward, sparse output): colour conversion, down-sampling, FDCT,
                   quantisation, masks, prefix sum, compaction
  copy_ms, floor   a device copy of the same frames, and frame bytes / 8 TB/s: what the device half is set against
  pcie_bytes       what crosses PCIe per frame in the sparse form (masks, offsets, used values), against raw_bytes, the frame itself
  host_fps         sv_jpeg_entropy_encode_batch on `threads` threads, records already in pinned memory
  e2e_fps          Context.imencode_batch, device tensor in, bytes out
  pillow_fps       Pillow (libjpeg-turbo) encoding the same frames on the same number of threads, including the D2H copy of the raw frames it needs
  d2h_fps          that raw D2H copy alone (into pinned memory)
Device figures are the median (min, max) over `windows` windows of HIP-event time per call (_timing.event_ms); host figures the median over
`windows` runs of the wall clock (_timing.wall_fps).  stream_wall_ms: host clock per frame of pipeline.recognize_stream(overlay=True) over 40 repeats of one synthetic 1080p frame with
encode off and on.
    python tools/time_jpeg_encode.py --stream-baseline --root PARENT_CHECKOUT [--json ...]
times the same loop without the encode argument on another (built) checkout: the parent commit's figure for "encode off".
Needs a GPU; there is no CPU path."""
import ctypes as C
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --root DIR: import the package from another checkout (the parent commit's, for --stream-baseline); read before the import below
PKG_ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv[:-1] else ROOT
sys.path.insert(0, PKG_ROOT)
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd import pipeline  # noqa: E402
from sudoku_vision_amd.synth import random_state_dict, synth_frames  # noqa: E402
import _timing  # noqa: E402

H, W = 1080, 1920
ITERS = {1: 400, 16: 40, 256: 3}


def solvable_grid():
    r, c = np.divmod(np.arange(81), 9)
    given = ((3 * (r % 3) + r // 3 + c) % 9 + 1).astype(np.uint8)
    given[np.random.RandomState(2).choice(81, 45, replace=False)] = 0
    return given


def contents(ctx):
    frame, corners, _ = synth_frames(1, H, W, seed=11, device="cuda")
    r, c = np.divmod(np.arange(81), 9)
    digits = torch.from_numpy(((3 * (r % 3) + r // 3 + c) % 9 + 1).astype(np.uint8)[None]).to(ctx.device)
    m, ok = sva.Context.corners_to_m_batch(np.asarray(corners, np.float32).reshape(1, 4, 2))
    assert ok.all()
    drawn = ctx.render_overlay(frame, ctx.minv_to_device(m), digits)[0]
    rgb = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "sample_1.jpg")).convert("RGB"))
    photo = np.tile(rgb[..., ::-1], (-(-H // rgb.shape[0]), -(-W // rgb.shape[1]), 1))[:H, :W]
    return {"synthetic_overlay": drawn, "photo_tiled": torch.from_numpy(np.ascontiguousarray(photo)).to(ctx.device)}


def host_only(ctx, frames, plan, threads):
    """the records of `frames` in pinned memory once; returns a closure that runs the host half alone"""
    n, nb = frames.shape[0], int(plan.info.coef_count) // 64
    masks, offsets, values, counts = ctx.jpeg_forward(frames, plan)
    used = [int(v) for v in counts.cpu().tolist()]
    pm, po = masks.cpu().pin_memory(), offsets.cpu().pin_memory()
    pv = [values[i, :max(u, 1)].cpu().pin_memory() for i, u in enumerate(used)]
    bounds = [int(ctx._lib.sv_jpeg_encode_bound(C.byref(plan), u)) for u in used]
    bufs = [np.empty(b, np.uint8) for b in bounds]
    VP = C.c_void_p * n
    args = (C.byref(plan), n, VP(*[pm.data_ptr() + 8 * nb * i for i in range(n)]), VP(*[po.data_ptr() + 4 * nb * i for i in range(n)]),
            VP(*[v.data_ptr() for v in pv]), (C.c_long * n)(*used), VP(*[b.ctypes.data for b in bufs]), (C.c_size_t * n)(*bounds), (C.c_size_t * n)(), threads,
            (C.c_int * n)())

    def run():
        assert ctx._lib.sv_jpeg_entropy_encode_batch(*args) == 0
    del masks, offsets, values
    pcie = 12 * nb + 4 + 2 * sum(used) / n                         # per frame: masks, offsets, the count word, the used values
    return run, (pm, po, pv, bufs), pcie


def stream_wall_ms(ctx, frame, given, encode, repeats=40):
    real = ctx.frames_to_digits
    logits = torch.full((1, 81, 10), -4.0, device=ctx.device)
    logits[0, torch.arange(81), torch.from_numpy(given.astype(np.int64))] = 6.0

    def reads_given(chunk, minv, out=None, **kw):                 # the recogniser as it is, then a solvable reading in place of its own
        r = real(chunk, minv, out=out, **kw)
        r["logits"].copy_(logits)
        r["digits"].copy_(logits.argmax(-1).to(torch.uint8))
        r["conf"].copy_(torch.softmax(logits, -1).max(-1).values)
        return r
    ctx.frames_to_digits = reads_given
    try:
        walls, sizes = [], []
        kw = {} if encode is None else {"encode": encode}           # None: a checkout from before the encoder has no such argument
        feed = pipeline.recognize_stream([frame] * repeats, ctx=ctx, glue=sva.Context.GLUE_NORMALIZE, overlay=True, **kw)
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = next(feed)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            if encode:
                sizes.append(len(r["jpeg"]))
        steady = walls[5:]
        return {"median": statistics.median(steady), "min": min(steady), "max": max(steady), "frames": len(steady),
                "jpeg_bytes_median": statistics.median(sizes) if sizes else None}
    finally:
        del ctx.frames_to_digits


def main():
    args = _timing.cli(__doc__, 5, [
        ("--threads", dict(type=int, default=16)),
        ("--root", dict(default=ROOT, help="checkout to import sudoku_vision_amd from")),
        ("--stream-baseline", dict(action="store_true", help="only recognize_stream(overlay=True) without the encode argument: the figure a checkout "
                                                             "from before the encoder gives (--root)"))])
    event_ms = lambda fn, iters: _timing.event_ms(fn, iters, args.windows, warmup=2)[:3]
    wall_fps = lambda fn, frames: _timing.wall_fps(fn, frames, args.windows, warmup=1)[:3]
    ctx = sva.default_context()
    if args.stream_baseline:
        frame = synth_frames(1, H, W, seed=11, device="cuda")[0][0]
        ctx.load_state_dict(random_state_dict(1234))
        res = {"what": "recognize_stream(overlay=True) wall ms per frame, one synthetic 1080p frame, no encode argument", "package": os.path.dirname(sva.__file__),
               "stream_wall_ms": {"overlay_only": stream_wall_ms(ctx, frame, solvable_grid(), None)}}
        _timing.emit(res, args.json)
        return
    res = {"what": "1080p BGR frames, 4:2:0; device: HIP-event ms per call, median (min, max) over windows; host: frames/s, median (min, max); one run",
           "windows": args.windows, "threads": args.threads, "raw_bytes": 3 * H * W, "cases": []}
    pool = ThreadPoolExecutor(args.threads)
    for name, frame in contents(ctx).items():
        host_frame = frame.cpu().numpy()
        for quality in (75, 95):
            plan = ctx.jpeg_encode_plan(W, H, 3, quality, "420", 0)
            want = None
            for n in (1, 16, 256):
                frames = frame[None].expand(n, H, W, 3).contiguous()
                dst = torch.empty_like(frames)
                pinned = torch.empty(frames.shape, dtype=torch.uint8).pin_memory()
                got = ctx.imencode_batch(frames[:1], quality, "420", 0, args.threads)[0]
                if want is None:
                    buf = io.BytesIO()
                    Image.fromarray(np.ascontiguousarray(host_frame[..., ::-1]), "RGB").save(buf, "JPEG", quality=quality, subsampling=2)
                    want = buf.getvalue()
                assert got == want, "the encoder's bytes are not Pillow's"
                case = {"content": name, "quality": quality, "frames": n, "file_bytes": len(got)}
                case["device_ms"] = event_ms(lambda: ctx.jpeg_forward(frames, plan), ITERS[n])
                case["copy_ms"] = event_ms(lambda: dst.copy_(frames), ITERS[n])
                case["floor_ms"] = _timing.floor_ms(frames.numel())
                case["device_over_copy"] = case["device_ms"][0] / case["copy_ms"][0]
                run, keep, case["pcie_bytes"] = host_only(ctx, frames, plan, args.threads)
                case["host_fps"] = wall_fps(run, n)
                del keep
                case["e2e_fps"] = wall_fps(lambda: ctx.imencode_batch(frames, quality, "420", 0, args.threads), n)

                def pillow():
                    pinned.copy_(frames, non_blocking=True)
                    torch.cuda.synchronize()
                    host = pinned.numpy()

                    def one(i):
                        b = io.BytesIO()
                        Image.fromarray(np.ascontiguousarray(host[i][..., ::-1]), "RGB").save(b, "JPEG", quality=quality, subsampling=2)
                        return b.getvalue()
                    return list(pool.map(one, range(n)))
                case["pillow_fps"] = wall_fps(pillow, n)
                case["d2h_fps"] = wall_fps(lambda: pinned.copy_(frames, non_blocking=True), n)
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
                del frames, dst, pinned
    frame = synth_frames(1, H, W, seed=11, device="cuda")[0][0]
    ctx.load_state_dict(random_state_dict(1234))
    res["stream_wall_ms"] = {"encode_off": stream_wall_ms(ctx, frame, solvable_grid(), False), "encode_on": stream_wall_ms(ctx, frame, solvable_grid(), True)}
    _timing.emit(res, args.json)


if __name__ == "__main__":
    main()
