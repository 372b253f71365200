#!/usr/bin/env python3
"""What the reduced-size JPEG decode (reduce = 2, 4, 8; csrc/k5_jpeg.hip) buys, against reduce = 1 of the same run.

    python tools/time_jpeg_reduced.py [--repeats 5] [--json profiles/jpeg_reduced_time.json]

Inputs: tests/golden/sample_1.jpg (3648 x 2736, 4:2:0) and 16 synthetic 1080p frames encoded on the spot (Pillow, quality 90, 4:2:0).
Per reduce, for each input: (a) the HIP-event time of the device half alone (coefficients already in HBM -> BGR frame), through the
compact and the dense transport; (b) imdecode_batch frames/s, host Huffman stage included (it decodes every coefficient at every
reduce); (c) on the photo, the wall time of recognize_image on the decoded frame, and whether it finds a grid.  Every timing is the
median of `repeats` windows after a warm-up (_timing.event_ms, _timing.wall_ms).  Each reduce runs in a child process of its own under a time limit; the first child that
fails ends the run.  Needs a GPU; there is no CPU path."""
import ctypes as C
import io
import json
import os
import subprocess
import sys

import _timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STEP_LIMIT_S = 240


def step(reduce, repeats):
    """one reduce, in this process -> dict"""
    import numpy as np
    import torch
    from PIL import Image
    sys.path.insert(0, ROOT)
    import sudoku_vision_amd as sva
    from sudoku_vision_amd import host
    from sudoku_vision_amd.pipeline import recognize_image
    from sudoku_vision_amd.synth import synth_frames

    ctx = sva.default_context()
    lib = sva._native.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def median_of(fn, iters, wall=False):
        if wall:
            return _timing.wall_ms(fn, repeats, warmup=2, iters=iters).median
        return _timing.event_ms(fn, iters, repeats, warmup=2).median

    def device_half_ms(data):
        """coefficients and quantiser steps of one file put into HBM once; then only the reconstruct entry is timed"""
        res = {}
        info = host.jpeg_parse(data)
        w, h = C.c_int(), C.c_int()
        sva._native.check(lib.sv_jpeg_scaled_size(C.byref(info), reduce, C.byref(w), C.byref(h)), "sv_jpeg_scaled_size")
        frame = torch.empty((h.value, w.value, 3), dtype=torch.uint8, device=ctx.device)
        _, coef, quant = host.jpeg_entropy_decode(data)
        dcoef, dquant = torch.from_numpy(coef).to(ctx.device), torch.from_numpy(quant.view(np.int16)).to(ctx.device)
        _, masks, offs, vals, _ = host.jpeg_entropy_decode_sparse(data)
        dm, do, dv = (torch.from_numpy(a.view(s)).to(ctx.device) for a, s in ((masks, np.int64), (offs, np.int32), (vals, np.int16)))
        p = lambda t: C.c_void_p(t.data_ptr())
        calls = {"dense": lambda: lib.sv_jpeg_reconstruct_scaled_bgr_u8(ctx._h, C.byref(info), p(dcoef), p(dquant), p(frame), frame.stride(0), stream(), reduce),
                 "sparse": lambda: lib.sv_jpeg_reconstruct_sparse_scaled_bgr_u8(ctx._h, C.byref(info), p(dm), p(do), p(dv), p(dquant), p(frame), frame.stride(0),
                                                                                stream(), reduce)}
        for name, call in calls.items():
            sva._native.check(call(), name)
            res[name + "_ms"] = median_of(call, 20)
        res["frame"] = [h.value, w.value]
        res["coefficient_bytes_dense"] = int(2 * coef.size)
        res["coefficient_bytes_sparse"] = int(12 * masks.size + 2 * vals.size)
        return res

    def batch_fps(datas, threads):
        ms = median_of(lambda: ctx.imdecode_batch(datas, threads=threads, reduce=reduce), 3, wall=True)
        return len(datas) * 1e3 / ms

    out = {"reduce": reduce, "device": torch.cuda.get_device_name()}
    photo = open(os.path.join(GOLDEN, "sample_1.jpg"), "rb").read()
    rec = {"file": "sample_1.jpg", "device_half": device_half_ms(photo), "imdecode_batch_fps": batch_fps([photo], 1)}
    g = np.load(os.path.join(GOLDEN, "cnn_coreml_fp16.npz"))
    keys = ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    ctx.load_state_dict({k: torch.from_numpy(g[k.replace(".", "_")].astype(np.float32)) for k in keys})
    frame = ctx.imdecode(photo, reduce=reduce)
    got = recognize_image(frame, ctx=ctx)
    rec["recognize_image_ms"] = median_of(lambda: recognize_image(frame, ctx=ctx), 3, wall=True)
    rec["grid_found"] = got is not None
    rec["digits_nonzero"] = None if got is None else int((got["digits"] != 0).sum())
    out["photo"] = rec

    frames, _, _ = synth_frames(16, 1080, 1920, seed=77)
    datas = []
    for f in frames.cpu().numpy():
        b = io.BytesIO()
        Image.fromarray(f[..., ::-1].copy()).save(b, "JPEG", quality=90, subsampling=2)
        datas.append(b.getvalue())
    out["synthetic_1080p"] = {"frames": 16, "mean_file_kB": sum(len(d) for d in datas) / 16e3, "device_half": device_half_ms(datas[0]),
                              "imdecode_batch_fps_16_threads": batch_fps(datas, 16)}
    return out


def main():
    args = _timing.cli(__doc__, None, [("--repeats", dict(type=int, default=5)),
                                       ("--step", dict(type=int, default=None, help="(internal) run one reduce in this process and print its record"))])
    if args.step is not None:
        print("RESULT " + json.dumps(step(args.step, args.repeats)), flush=True)
        return 0
    out = {"repeats": args.repeats, "steps": []}
    for reduce in (1, 2, 4, 8):
        try:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(reduce), "--repeats", str(args.repeats)],
                                   capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"reduce={reduce}: no result within {STEP_LIMIT_S} s; stopping", flush=True)
            return 1
        lines = [ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")]
        if child.returncode != 0 or not lines:
            print(f"reduce={reduce}: exit status {child.returncode}; stopping\n{child.stderr[-2000:]}", flush=True)
            return 1
        rec = json.loads(lines[-1][7:])
        out["device"] = rec.pop("device")
        out["steps"].append(rec)
        print(json.dumps(rec), flush=True)
    base = out["steps"][0]
    out["against_reduce_1"] = [{"reduce": r["reduce"],
                                "photo_device_half_sparse": base["photo"]["device_half"]["sparse_ms"] / r["photo"]["device_half"]["sparse_ms"],
                                "photo_device_half_dense": base["photo"]["device_half"]["dense_ms"] / r["photo"]["device_half"]["dense_ms"],
                                "photo_imdecode_batch_fps": r["photo"]["imdecode_batch_fps"] / base["photo"]["imdecode_batch_fps"],
                                "photo_recognize_image": base["photo"]["recognize_image_ms"] / r["photo"]["recognize_image_ms"],
                                "synthetic_device_half_sparse": base["synthetic_1080p"]["device_half"]["sparse_ms"] / r["synthetic_1080p"]["device_half"]["sparse_ms"],
                                "synthetic_imdecode_batch_fps": r["synthetic_1080p"]["imdecode_batch_fps_16_threads"] / base["synthetic_1080p"]["imdecode_batch_fps_16_threads"]}
                               for r in out["steps"]]
    _timing.emit(out, args.json)
    return 0


if __name__ == "__main__":
    sys.exit(main())
