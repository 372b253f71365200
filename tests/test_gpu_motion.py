"""K15 (csrc/k15_motion.hip), Context.motion_update, cv/stabilizer.py's MotionDetector and pipeline.recognize_stream on the GPU
against tests/stabilizer_ref.py: small images bit for bit, counts exactly."""
import numpy as np
import pytest
import torch

import stabilizer_ref as R

pytestmark = pytest.mark.gpu

TOL = 4e-3          # tests/test_stabilizer_ref.py: six float32 roundings of coordinates below 4096
SHAPES = [(1, 1), (5, 7), (119, 161), (120, 160), (240, 320), (240, 321), (241, 320), (251, 333), (1080, 1920)]


def _noise(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def _structured(shape, phase):
    """A gradient with a checkerboard on top: edges at every scale, nothing random."""
    H, W = shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    img = ((xx * 3 + yy * 5 + phase * 40) % 256 + (((yy // 3 + xx // 5 + phase) % 2) * 90)) % 256
    img = img.astype(np.uint8)
    return img if len(shape) == 2 else np.stack([img, np.roll(img, 7, 1), 255 - img], -1)


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _check(ctx, frames, prev=None, threshold=30.0, dsize=(160, 120), dev_frames=None):
    """frames: numpy [n,H,W(,3)]; dev_frames: the same frames as a device tensor in some layout."""
    want_small, want_counts = R.motion_counts(frames, prev, threshold, dsize)
    small, counts = ctx.motion_update(_dev(ctx, frames) if dev_frames is None else dev_frames, None if prev is None else _dev(ctx, prev), threshold, dsize)
    assert small.dtype == torch.uint8 and tuple(small.shape) == want_small.shape and counts.dtype == torch.int32
    got = small.cpu().numpy()
    bad = np.argwhere(got != want_small)
    assert bad.size == 0, f"{len(bad)} small pixels differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want_small[tuple(bad[0])]}"
    assert counts.cpu().numpy().tolist() == want_counts.tolist()
    return want_small, want_counts


# ---- shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_noise_and_structure(ctx, shape, channels):
    full = shape + ((3,) if channels == 3 else ())
    frames = np.stack([_noise(full, 1 + sum(shape)), _structured(full, 0), _structured(full, 1), _noise(full, 2 + sum(shape))])
    prev = _noise((120, 160), 5)
    _, counts = _check(ctx, frames, prev)
    if shape != (1, 1):
        assert counts.min() > 0                            # the cases do exercise the count
    _check(ctx, frames[1:2])                               # one frame, no previous one: counts[0] == 0


def test_padded_rows_from_an_odd_base_address(ctx):
    H, W = 251, 333
    frames = np.stack([_noise((H, W, 3), 11), _structured((H, W, 3), 2)])
    raw = torch.full((2 * (H + 3) * (W * 3 + 38) + 1,), 255, dtype=torch.uint8, device=ctx.device)
    view = raw[1:].view(2, H + 3, W * 3 + 38)[:, :H, :W * 3].unflatten(2, (W, 3))
    view.copy_(_dev(ctx, frames))
    assert view.data_ptr() % 2 == 1 and view.stride(1) == W * 3 + 38 and not view.is_contiguous()
    _check(ctx, frames, _noise((120, 160), 12), dev_frames=view)
    gray = np.stack([_noise((H, W), 13), _structured((H, W), 3)])
    rawg = torch.zeros((2 * (H + 1) * (W + 9) + 1,), dtype=torch.uint8, device=ctx.device)
    viewg = rawg[1:].view(2, H + 1, W + 9)[:, :H, :W]
    viewg.copy_(_dev(ctx, gray))
    _check(ctx, gray, None, dev_frames=viewg)


def test_gapped_batch_of_three(ctx):
    H, W = 119, 161
    frames = np.stack([_noise((H, W, 3), 21 + i) for i in range(3)])
    buf = torch.zeros((3, H + 17, W, 3), dtype=torch.uint8, device=ctx.device)
    view = buf[:, :H]
    view.copy_(_dev(ctx, frames))
    assert view.stride(0) > H * view.stride(1)
    _check(ctx, frames, _noise((120, 160), 20), dev_frames=view)


@pytest.mark.parametrize("dsize", [(13, 7), (1, 1), (160, 120)])
def test_other_target_sizes(ctx, dsize):
    frames = np.stack([_noise((97, 203, 3), 31), _structured((97, 203, 3), 1), _noise((97, 203, 3), 32)])
    prev = _noise((dsize[1], dsize[0]), 33)
    _check(ctx, frames, prev, dsize=dsize)
    exact2 = np.stack([_noise((2 * dsize[1], 2 * dsize[0]), 34), _noise((2 * dsize[1], 2 * dsize[0]), 35)])
    _check(ctx, exact2, prev, dsize=dsize)                 # the 2x2 area rule at this size


def test_both_launch_shapes_agree(ctx):
    """The cross-check library's two-launch shape against the restatement and the product's single launch."""
    import sudoku_vision_amd as sva
    xlib = sva._native.lib_xcheck()
    xc = sva.Context(ctx.device, library=xlib)
    frames = np.stack([_noise((251, 333, 3), 41 + i) for i in range(4)])
    prev = _noise((120, 160), 40)
    try:
        one = _check(xc, frames, prev)
        xc._check(xlib.svx_ctx_set_motion_shape(xc._h, 1), "svx_ctx_set_motion_shape")
        two = _check(xc, frames, prev)
        _check(xc, frames[:1], None)
        assert xlib.svx_ctx_set_motion_shape(xc._h, 7) == -1
    finally:
        xc.close()
    assert (one[0] == two[0]).all() and (one[1] == two[1]).all()


# ---- thresholds --------------------------------------------------------------------------------------------------------------
def _tie_frames():
    a = np.full((120, 160), 100, np.uint8)
    b = a.copy()
    b.reshape(-1)[[63, 64, 300, 5000, 12345, 19136, 19199]] = 130          # differences of exactly 30
    b.reshape(-1)[[0, 127, 255, 256, 511, 700, 9000, 9001, 15000, 19000, 19198]] = 69     # 31, downwards
    return a, b


@pytest.mark.parametrize("threshold,want", [(30.0, 11), (30.5, 11), (31.0, 0), (29.5, 18), (30.0 - 1e-12, 18), (255, 0), (1e9, 0), (-1, 19200),
                                            (-0.25, 19200), (0.0, 18)])
def test_threshold_ties(ctx, threshold, want):
    a, b = _tie_frames()
    _, counts = _check(ctx, b[None], a, threshold)
    assert counts.tolist() == [want]
    _, counts = _check(ctx, np.stack([a, b, b]), None, threshold)          # the same through the in-batch previous frame
    assert counts.tolist() == [0, want, 19200 if threshold < 0 else 0]


def _changed(npx):
    """npx pixel indices spread over the 75 workgroups of a 160x120 image, last lanes of waves among them."""
    idx = (np.arange(npx) * 101 + 63) % 19200
    assert len(set(idx.tolist())) == npx and (idx % 64 == 63).sum() >= 2 and len(set((idx // 256).tolist())) > 8
    return idx


@pytest.mark.parametrize("npx,want", [(192, False), (193, True)])
def test_ratio_ties(ctx, npx, want):
    from sudoku_vision_amd.cv.stabilizer import MotionDetector
    a = np.full((120, 160), 10, np.uint8)
    b = a.copy()
    b.reshape(-1)[_changed(npx)] = 200
    for frames in ((a, b), (_dev(ctx, a), _dev(ctx, b))):                   # numpy and device frames
        d = MotionDetector()
        assert d.prev_frame is None
        assert d.update(frames[0]) is False
        assert d.update(frames[1]) is want
        assert (d.prev_frame == b).all()
        assert d.update(frames[1]) is False                 # the previous frame was replaced, motion or not
    _, counts = ctx.motion_update(_dev(ctx, b[None]), _dev(ctx, a))
    assert int(counts[0]) == npx


# ---- the detector's sequence semantics -----------------------------------------------------------------------------------------
def test_update_batch_equals_updates_and_state_carries(ctx):
    from sudoku_vision_amd.cv.stabilizer import MotionDetector
    base = _structured((251, 333, 3), 0)
    feed = [base, base, _structured((251, 333, 3), 1), _structured((251, 333, 3), 1), _noise((251, 333, 3), 50), base, base]
    ref = R.Detector()
    want = [ref.update(f) for f in feed]
    assert want[0] is False and True in want and False in want[1:]
    one = MotionDetector()
    got_one = [one.update(f) for f in feed]
    assert got_one == want and all(isinstance(v, bool) for v in got_one)
    batched = MotionDetector()
    got = list(batched.update_batch(np.stack(feed[:2]))) + list(batched.update_batch(_dev(ctx, np.stack(feed[2:]))))
    assert got == want
    assert batched.update_batch(np.stack(feed[:1])).dtype == np.bool_
    assert (one.prev_frame == ref.prev_frame).all()
    one.update(feed[0])
    assert (batched.prev_frame == one.prev_frame).all()
    gray = MotionDetector()
    g = [f[..., 1] for f in feed]                          # gray frames take the same path without the conversion
    refg = R.Detector()
    assert [gray.update(f) for f in g] == [refg.update(f) for f in g]
    gray.prev_frame = None                                  # restarts the feed
    assert gray.update(g[4]) is False


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import sudoku_vision_amd as sva
    ok = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.motion_update(ok[0, 0])                                        # rank 2
    with pytest.raises(ValueError):
        ctx.motion_update(torch.zeros((1, 8, 8, 2), dtype=torch.uint8, device=ctx.device))
    with pytest.raises(ValueError):
        ctx.motion_update(ok.float())
    with pytest.raises(ValueError):
        ctx.motion_update(ok.cpu())
    with pytest.raises(ValueError):
        ctx.motion_update(ok, prev_small=torch.zeros((160, 120), dtype=torch.uint8, device=ctx.device))
    with pytest.raises(ValueError):
        ctx.motion_update(ok, prev_small=torch.zeros((120, 160), dtype=torch.int32, device=ctx.device))
    with pytest.raises(TypeError):
        ctx.motion_update(ok, out=(torch.zeros((1, 120, 161), dtype=torch.uint8, device=ctx.device), None))
    lib = sva._native.lib()
    small = torch.zeros((1, 120, 160), dtype=torch.uint8, device=ctx.device)
    counts = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    args = lambda ch, H=8, fr=ok, sm=small, cn=counts, prev=None: (ctx._h, fr.data_ptr() if fr is not None else None, 1, H, 8, ch, 24, 192, prev,  # noqa: E731
                                                                    30.0, sm.data_ptr() if sm is not None else None, cn.data_ptr() if cn is not None else None, 120, 160, None)
    assert lib.sv_motion_update_u8(*args(2)) == -1 and b"channels" in lib.sv_last_error()
    assert lib.sv_motion_update_u8(*args(3, H=0)) == -1
    assert lib.sv_motion_update_u8(*args(3, sm=None)) == -1 and lib.sv_motion_update_u8(*args(3, cn=None)) == -1
    assert lib.sv_motion_update_u8(*args(3, prev=small.data_ptr())) == -1 and b"overlaps" in lib.sv_last_error()
    assert lib.sv_motion_update_u8(*args(3)) == 0
    torch.cuda.synchronize()


# ---- the feed loop -----------------------------------------------------------------------------------------------------------
def test_recognize_stream(ctx):
    import cnn_oracle
    from sudoku_vision_amd import Context, pipeline
    from sudoku_vision_amd.cv.stabilizer import GridStabilizer
    from sudoku_vision_amd.synth import synth_frames
    frames, _, _ = synth_frames(1, 270, 480, seed=11, device="cpu")
    f0 = frames[0].numpy()
    blank = np.full_like(f0, 128)
    sd = cnn_oracle.random_state_dict(1234)
    want = pipeline.recognize_image(f0, sd, ctx=ctx, glue=Context.GLUE_NORMALIZE)
    assert want is not None
    feed = [f0, _dev(ctx, f0), f0, 255 - f0, blank, blank]
    got = list(pipeline.recognize_stream(feed, sd, ctx=ctx, glue=Context.GLUE_NORMALIZE))
    assert [r["motion"] for r in got] == [False, False, False, True, True, False]
    for r in got[:2]:                                       # use_kalman=True: zero corners before min_detections, no homography
        assert r["detected"] and not r["stabilized"].is_stable and (r["stabilized"].corners == 0).all()
        assert (r["stabilized"].raw_corners == want["corners"]).all()
        assert r["digits"] is None and r["corners_used"] is None and r["confidence"] is None
    third = got[2]
    assert third["detected"] and third["stabilized"].is_stable and third["stabilized"].frames_detected == 3
    assert np.abs(third["corners_used"] - want["corners"]).max() <= TOL
    assert (np.rint(third["corners_used"]) == want["corners"]).all()
    assert (third["digits"] == want["digits"]).all() and third["confidence"].shape == (81,)
    for r in got[3:5]:                                      # skipped: the stabiliser did not see them
        assert r["stabilized"] is None and r["digits"] is None and not r["detected"]
    last = got[5]
    assert not last["detected"] and not last["stabilized"].is_stable and last["stabilized"].frames_detected == 2
    assert last["stabilized"].corners is third["stabilized"].corners          # the last stable corners, while the history lasts
    # without the filters the first detections are used as they are
    plain = list(pipeline.recognize_stream([f0, f0], sd, ctx=ctx, glue=Context.GLUE_NORMALIZE, stabilizer=GridStabilizer(use_kalman=False)))
    assert all((r["digits"] == want["digits"]).all() and (r["corners_used"] == want["corners"]).all() for r in plain)
    with pytest.raises(ValueError):
        next(pipeline.recognize_stream([f0], grid="v3"))
