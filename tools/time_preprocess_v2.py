"""Timing of run_v2's preprocessing (csrc/k7_preprocess_v2.hip, cv/preprocess_v2.py) at 16 x 1080p and at one 3648x2736 photo.

    python tools/time_preprocess_v2.py [--iters 20] [--repeats 5] [--json out.json]

Per stage: HIP-event time per call (_timing.event_ms: median of `repeats` windows of `iters` calls, after a warm-up that also ramps the clock)
beside the bytes the stage must move (every input read once, every output written once) over the 8 TB/s HBM peak, and beside
K1 (sv_preprocess_u8) on the same frames.  preprocess_multi_strategy as a whole is a host clock around one call per frame ending
in a synchronise (it takes decisions on the host between stages).  normalize_illumination at k = 51 and k = 193 on the same
1080p frames shows how the large close scales with k.  Needs a GPU; there is no CPU path."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd.cv import preprocess_v2  # noqa: E402
from sudoku_vision_amd.synth import synth_frames  # noqa: E402
from _timing import HBM_PEAK_BYTES_PER_S, cli, emit, event_ms, floor_ms, wall_ms  # noqa: E402


def stages(ctx, gray, bgr, iters, repeats):
    """gray u8 [n,H,W], bgr u8 [n,H,W,3] on device -> {stage: {ms, bytes, floor_ms, x_floor}}."""
    n, H, W = gray.shape
    px = n * H * W
    k_illum, k_shadow = preprocess_v2.illumination_kernel_size((H, W)), preprocess_v2.shadow_kernel_size((H, W))
    other = ctx.box_mean(gray, k_shadow)
    binary = ctx.threshold_sauvola(gray, 25, 0.2)
    table = [
        ("K1 sv_preprocess_u8 (for scale)", lambda: ctx.preprocess(bgr), 4 * px),
        (f"close ELLIPSE {k_illum} (normalize_illumination)", lambda: ctx.morphology(gray, ctx.MORPH_CLOSE, ctx.SHAPE_ELLIPSE, k_illum), 2 * px),
        ("dilate ELLIPSE 7 (remove_shadow)", lambda: ctx.morphology(gray, ctx.MORPH_DILATE, ctx.SHAPE_ELLIPSE, 7), 2 * px),
        ("close RECT 3 + open RECT 2 (cleanup)", lambda: ctx.morphology(ctx.morphology(binary, ctx.MORPH_CLOSE, ctx.SHAPE_RECT, 3), ctx.MORPH_OPEN,
                                                                          ctx.SHAPE_RECT, 2), 4 * px),
        (f"box mean {k_shadow} (detect_shadow)", lambda: ctx.box_mean(gray, k_shadow), 2 * px),
        ("GaussianBlur 21", lambda: ctx.gaussian_blur21(gray), 2 * px),
        ("divide", lambda: ctx.divide_normalize(gray, other), 3 * px),
        ("CLAHE 2.0 8x8", lambda: ctx.clahe(gray, 2.0, (8, 8)), 3 * px),
        ("Sauvola 25", lambda: ctx.threshold_sauvola(gray, 25, 0.2), 2 * px),
        ("threshold + count", lambda: ctx.threshold_count(gray, 127, inv=True), 2 * px),
        ("shadow mask + count", lambda: ctx.shadow_mask(gray, other), 3 * px),
        ("count_nonzero", lambda: ctx.count_nonzero(binary), px),
    ]
    res = {}
    for name, fn, nbytes in table:
        ms = event_ms(fn, iters, repeats, warmup=3).median
        floor = floor_ms(nbytes)
        res[name] = {"ms": ms, "bytes": nbytes, "floor_ms_at_8TBps": floor, "x_floor": ms / floor}
    return res


def whole(frames, repeats):
    """preprocess_multi_strategy, one call per frame, host clock to a synchronise -> median ms per frame."""
    last = []

    def every_frame():
        for f in frames:
            last[:] = [preprocess_v2.preprocess_multi_strategy(f)]
    return wall_ms(every_frame, repeats, warmup=1).median / len(frames), last[0]


def main():
    photo = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "sample_4.jpg")
    args = cli(__doc__, None, [("--iters", dict(type=int, default=20)), ("--repeats", dict(type=int, default=5)), ("--photo", dict(default=photo))])
    ctx = sva.default_context()
    res = {"iters": args.iters, "repeats": args.repeats, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S}

    frames, _, _ = synth_frames(16, 1080, 1920, seed=1234, device="cuda")
    gray = ctx.gray(frames)
    res["16x1080p"] = stages(ctx, gray, frames, args.iters, args.repeats)
    ms, r = whole(list(frames), args.repeats)
    res["16x1080p"]["preprocess_multi_strategy (per frame, host clock)"] = {"ms": ms, "method_used": r.method_used, "has_shadow": r.has_shadow}
    one = gray[:1]
    scale = {}
    for k in (51, 193):
        background = ctx.morphology(one, ctx.MORPH_CLOSE, ctx.SHAPE_ELLIPSE, k)
        scale[str(k)] = event_ms(lambda: ctx.divide_normalize(one, ctx.morphology(one, ctx.MORPH_CLOSE, ctx.SHAPE_ELLIPSE, k)), args.iters, args.repeats,
                                 warmup=3).median
        del background
    res["normalize_illumination_1x1080p_ms_by_k"] = dict(scale, ratio_193_over_51=scale["193"] / scale["51"], k_ratio=193 / 51)
    del frames, gray, one

    from sudoku_vision_amd import imgcodecs
    photo = imgcodecs.imread(args.photo, device=True, ctx=ctx)
    if photo is None:
        raise SystemExit(f"cannot read {args.photo}")
    res["photo_shape"] = list(photo.shape)
    res["1xphoto"] = stages(ctx, ctx.gray(photo[None]), photo[None], max(2, args.iters // 4), args.repeats)
    ms, r = whole([photo], args.repeats)
    res["1xphoto"]["preprocess_multi_strategy (per frame, host clock)"] = {"ms": ms, "method_used": r.method_used, "has_shadow": r.has_shadow}
    emit(res, args.json)


if __name__ == "__main__":
    main()
