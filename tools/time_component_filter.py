"""What K11, the component filter (csrc/k11_components.hip), buys the host corner search: the committed photos at full size and 16
synthetic 1080p frames.

    python tools/time_component_filter.py [--repeats 5] [--json out.json]

Per frame, all in this process: (a) the host search on one thread behind K4 alone (the path without K11), (b) K11's HIP-event time on the
K4 output, (c) the host search behind K4 + K11, (d) the bytes that cross to the host before and after (dense bytes or bits; non-zero
32-bit words of the bit image, what a sparse record would carry), (e) the 8-connected components before and after.  Every timing is the
median of `repeats` windows after a warm-up (_timing.event_ms for the device, _timing.wall_ms for the host).  The claim to check is (b) + (c) < (a).  Needs a GPU; there is no CPU path."""
import glob
import json
import os
import statistics
import sys

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd import host, imgcodecs  # noqa: E402
from sudoku_vision_amd.synth import synth_frames  # noqa: E402
import _timing  # noqa: E402

RATIO = 0.1


def device_ms(fn, iters, repeats):
    return _timing.event_ms(fn, iters, repeats, warmup=3).median


def host_ms(fn, iters, repeats):
    return _timing.wall_ms(fn, repeats, warmup=1, sync=False, iters=iters).median


def components(img):
    return int(ndimage.label(img != 0, structure=np.ones((3, 3), bool))[1])


def measure(ctx, frames, repeats, iters):
    """frames u8 [n,H,W,3] on the device -> one record per frame (times per frame)."""
    n, H, W = frames.shape[:3]
    k4 = ctx.despeckle(ctx.preprocess(frames)) if RATIO * H * W > 61 * 61 else ctx.preprocess(frames)
    work = torch.empty_like(k4)
    t_copy = device_ms(lambda: work.copy_(k4), iters, repeats)
    bits_form = W % 32 == 0
    if bits_form:
        packed = torch.empty((n, H, W // 32), dtype=torch.int32, device=frames.device)
        ctx.component_filter(k4, 0.0, packed=packed)                          # ratio 0: a plain pack of K4's output
        wbits = torch.empty_like(packed)
        t_copyb = device_ms(lambda: wbits.copy_(packed), iters, repeats)
        t_k11 = device_ms(lambda: ctx.component_filter_bits(wbits.copy_(packed), RATIO), iters, repeats) - t_copyb
        after_bits = ctx.component_filter_bits(wbits.copy_(packed), RATIO).cpu().numpy()
        before_bits = packed.cpu().numpy()
    t_k11_u8 = device_ms(lambda: ctx.component_filter(work.copy_(k4), RATIO, out=work), iters, repeats) - t_copy
    after = ctx.component_filter(k4, RATIO).cpu().numpy()
    before = k4.cpu().numpy()
    recs = []
    for f in range(n):
        if bits_form:
            search = lambda b: host.find_grid_corners_bits_batch(b[f:f + 1], H, W, RATIO, threads=1)
            (ca, fa), (cb, fb) = search(before_bits), search(after_bits)
            same = bool(fa[0] == fb[0] and (not fa[0] or (ca[0] == cb[0]).all()))
            a_ms, c_ms = host_ms(lambda: search(before_bits), iters, repeats), host_ms(lambda: search(after_bits), iters, repeats)
            d2h = {"before_bytes": H * W // 8, "after_bytes": H * W // 8, "before_nonzero_words": int((before_bits[f] != 0).sum()),
                   "after_nonzero_words": int((after_bits[f] != 0).sum())}
        else:
            ca, cb = host.find_grid_corners(before[f], RATIO), host.find_grid_corners(after[f], RATIO)
            same = (ca is None) == (cb is None) and (ca is None or bool((ca == cb).all()))
            a_ms = host_ms(lambda: host.find_grid_corners(before[f], RATIO), iters, repeats)
            c_ms = host_ms(lambda: host.find_grid_corners(after[f], RATIO), iters, repeats)
            d2h = {"before_bytes": H * W, "after_bytes": H * W, "before_nonzero_bytes": int((before[f] != 0).sum()), "after_nonzero_bytes": int((after[f] != 0).sum())}
        b_ms = (t_k11 if bits_form else t_k11_u8) / n
        recs.append({"H": H, "W": W, "form": "bits" if bits_form else "bytes", "a_host_search_behind_k4_ms": a_ms, "b_k11_ms": b_ms,
                     "b_k11_byte_entry_ms": t_k11_u8 / n, "c_host_search_behind_k4_k11_ms": c_ms, "b_plus_c_ms": b_ms + c_ms,
                     "b_plus_c_below_a": bool(b_ms + c_ms < a_ms), "d2h": d2h, "components_before": components(before[f]),
                     "components_after": components(after[f]), "same_corners": same})
    return recs


def main():
    args = _timing.cli(__doc__, None, [("--repeats", dict(type=int, default=5)), ("--iters", dict(type=int, default=3))])
    ctx = sva.default_context()
    out = {"ratio": RATIO, "repeats": args.repeats, "iters": args.iters, "device": torch.cuda.get_device_name(), "photos": [], "synthetic_1080p": None}
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    for path in sorted(glob.glob(os.path.join(golden, "sample_*.jpg"))):
        frame = imgcodecs.imread(path, device=True, ctx=ctx)
        rec = measure(ctx, frame[None].contiguous(), args.repeats, args.iters)[0]
        rec["file"] = os.path.basename(path)
        out["photos"].append(rec)
        print(json.dumps(rec), flush=True)
    frames, _, _ = synth_frames(16, 1080, 1920, seed=0)
    recs = measure(ctx, frames.to(ctx.device), args.repeats, args.iters)
    med = lambda k: statistics.median(r[k] for r in recs)
    out["synthetic_1080p"] = {"frames": 16, "a_host_search_behind_k4_ms": med("a_host_search_behind_k4_ms"), "b_k11_ms": med("b_k11_ms"),
                              "c_host_search_behind_k4_k11_ms": med("c_host_search_behind_k4_k11_ms"), "components_before": med("components_before"),
                              "components_after": med("components_after"), "same_corners": all(r["same_corners"] for r in recs),
                              "b_plus_c_below_a": bool(med("b_k11_ms") + med("c_host_search_behind_k4_k11_ms") < med("a_host_search_behind_k4_ms"))}
    print(json.dumps(out["synthetic_1080p"]), flush=True)
    out["claim_b_plus_c_below_a_on_every_photo"] = all(r["b_plus_c_below_a"] for r in out["photos"])
    _timing.emit(out, args.json)
    print("claim (b) + (c) < (a) on every photo:", out["claim_b_plus_c_below_a_on_every_photo"])


if __name__ == "__main__":
    main()
