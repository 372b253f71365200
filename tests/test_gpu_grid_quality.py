"""GPU (-m gpu): the quality gate's kernels (csrc/k6_quality.hip) bit-exact against numpy / oracle statistics, and the
cv.grid_quality drop-in and FramePipeline(quality=True) end to end."""
import os

import numpy as np
import pytest
import torch

import quality_ref as R
import sv_oracle
from sudoku_vision_amd import host
from sudoku_vision_amd.cv import grid_quality as gq
from sudoku_vision_amd.pipeline import FramePipeline
from sudoku_vision_amd.runtime import Context
from sudoku_vision_amd.synth import synth_frames, random_state_dict

pytestmark = pytest.mark.gpu


def _photos(golden_dir):
    out = []
    for k in range(1, 6):
        with open(os.path.join(golden_dir, f"sample_{k}.jpg"), "rb") as fh:
            out.append(sv_oracle.imdecode(fh.read()))
    return out


def _check_stats(ctx, dev_frames, host_frames):
    s1, s2, hist = ctx.frame_quality_stats(dev_frames)
    s1, s2, hist = s1.cpu().numpy(), s2.cpu().numpy(), hist.cpu().numpy()
    for f, img in enumerate(host_frames):
        e1, e2, eh, _ = R.frame_stats(img)
        assert (s1[f], s2[f]) == (e1, e2), (f, img.shape)
        assert (hist[f] == eh).all(), (f, img.shape)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (17, 33), (33, 1025), (40, 2049)])
@pytest.mark.parametrize("channels", [1, 3])
def test_stats_small_shapes(ctx, shape, channels):
    H, W = shape
    rs = np.random.RandomState(H * 1000 + W + channels)
    imgs = rs.randint(0, 256, (3, H, W, 3) if channels == 3 else (3, H, W)).astype(np.uint8)
    _check_stats(ctx, torch.from_numpy(imgs).cuda(), imgs)


@pytest.mark.parametrize("channels", [1, 3])
def test_stats_padded_pitch_and_gaps(ctx, channels):
    rs = np.random.RandomState(7)
    H, W = 37, 61
    # rows padded to 13 extra pixels, 5 spare rows between frames, odd base offset: the byte path
    big = torch.from_numpy(rs.randint(0, 256, (4, H + 5, W + 13, 3)).astype(np.uint8)).cuda()
    view = big[:, 2:2 + H, 1:1 + W] if channels == 3 else big[:, 2:2 + H, 1:1 + W, 0]
    _check_stats(ctx, view, view.cpu().numpy())
    # 16-byte aligned pitch and frame stride with gaps: the vector path (W2 = 3 * 16 + 5 px: full lane groups and a partial one)
    W2 = 53
    shape = (3, H + 3, W2 + 11, 3) if channels == 3 else (3, H + 3, W2 + 11)
    big = torch.from_numpy(rs.randint(0, 256, shape).astype(np.uint8)).cuda()
    view = big[:, :H, :W2]
    assert view.stride(1) % 16 == 0 and view.stride(0) % 16 == 0
    _check_stats(ctx, view, view.cpu().numpy())


def test_stats_1080p_batch(ctx):
    frames, _, _ = synth_frames(64, 1080, 1920, seed=3, device="cuda")
    _check_stats(ctx, frames, frames.cpu().numpy())


def test_stats_photos(ctx, golden_dir):
    for img in _photos(golden_dir):
        _check_stats(ctx, torch.from_numpy(img).cuda()[None], img[None])


def _coverage_both(ctx, binary, corners):
    minv, ok = Context.corners_to_minv_batch(np.asarray(corners, np.float32), 450)
    md = ctx.minv_to_device(minv)
    b = torch.from_numpy(np.ascontiguousarray(binary)).cuda()
    c8 = ctx.grid_line_coverage(b, md).cpu().numpy()
    cb = None
    if binary.shape[2] % 32 == 0:
        bits = np.packbits(binary > 0, axis=2, bitorder="little").view(np.int32)
        cb = ctx.grid_line_coverage(torch.from_numpy(np.ascontiguousarray(bits)).cuda(), md).cpu().numpy()
    return c8, cb, ok


def test_coverage_synthetic(ctx):
    frames, corners, _ = synth_frames(8, 540, 960, seed=9, noise="int")
    host_frames = frames.numpy()
    binary = np.stack([sv_oracle.preprocess_for_grid_detection(f) for f in host_frames])
    # two frames with corners partly outside the frame
    corners = corners.copy()
    corners[1] += np.array([[-300, -120], [0, 0], [0, 0], [0, 0]], np.float32)
    corners[2, 2] += np.array([400, 250], np.float32)
    c8, cb, ok = _coverage_both(ctx, binary, corners)
    assert ok.all()
    for f in range(len(binary)):
        exp = R.coverage_counts(binary[f], corners[f])
        assert (c8[f] == exp).all(), f
        assert (cb[f] == exp).all(), f


def test_coverage_gray_levels(ctx):
    # values other than 0/255: a warped pixel between small taps can round to 0, which the kernel must not shortcut
    rs = np.random.RandomState(4)
    img = (rs.randint(0, 3, (2, 300, 320)) * rs.randint(0, 2, (2, 300, 320))).astype(np.uint8)
    corners = np.array([[[20, 10], [300, 30], [290, 280], [5, 290]], [[40, 40], [250, 20], [280, 260], [30, 250]]], np.float32)
    c8, _, _ = _coverage_both(ctx, img[:, :, :300], corners)
    for f in range(2):
        assert (c8[f] == R.coverage_counts(img[f, :, :300], corners[f])).all()


def test_coverage_degenerate_quad(ctx):
    frames, corners, _ = synth_frames(2, 540, 960, seed=2, noise="int")
    binary = np.stack([sv_oracle.preprocess_for_grid_detection(f) for f in frames.numpy()])
    corners = corners.copy()
    corners[0] = [[480, 20], [740, 270], [480, 520], [220, 270]]          # rotated 45 degrees
    c8, cb, ok = _coverage_both(ctx, binary, corners)
    assert not ok[0] and ok[1]
    # identity matrix for the degenerate frame: the bands of the top-left 450x450 crop
    assert (c8[0] == R.warped_counts(binary[0][:450, :450])).all() and (cb[0] == c8[0]).all()
    assert (c8[1] == R.coverage_counts(binary[1], corners[1])).all() and (cb[1] == c8[1]).all()
    q = gq.assess_grid_quality_batch(ctx, frames.cuda(), torch.from_numpy(binary).cuda(), corners, [True, True])
    assert np.isnan(q[0, [0, 3, 4, 5]]).all() and np.isfinite(q[0, 1:3]).all() and np.isfinite(q[1]).all()


def test_coverage_photos(ctx, golden_dir):
    for img in _photos(golden_dir):
        binary = sv_oracle.preprocess_for_grid_detection(img)
        corners = host.find_grid_corners(binary)
        if corners is None:
            continue
        c8, cb, ok = _coverage_both(ctx, binary[None], corners[None].astype(np.float32))
        exp = R.coverage_counts(binary, corners.astype(np.float32))
        assert ok[0] and (c8[0] == exp).all()
        assert cb is None or (cb[0] == exp).all()


def test_assess_grid_quality_matches_reference(ctx, golden_dir):
    frames, corners, _ = synth_frames(3, 540, 960, seed=21, noise="int")
    cases = [(f, sv_oracle.preprocess_for_grid_detection(f), c) for f, c in zip(frames.numpy(), corners)]
    for img in _photos(golden_dir):
        binary = sv_oracle.preprocess_for_grid_detection(img)
        c = host.find_grid_corners(binary)
        if c is not None:
            cases.append((img, binary, c.astype(np.float32)))
    for img, binary, c in cases:
        q = gq.assess_grid_quality(img, binary, c)
        r = R.ref_assess(img, binary, c)
        R.compare(q, r)
        if not R.near_threshold(r):
            assert gq.get_user_feedback(q) == r["feedback"]
        # CUDA tensors in, the same result
        q2 = gq.assess_grid_quality(torch.from_numpy(img).cuda(), torch.from_numpy(binary).cuda(), torch.from_numpy(c))
        assert q2 == q
        assert gq.compute_sharpness(sv_oracle.gray(img)) == q.sharpness
        assert gq.compute_contrast(torch.from_numpy(sv_oracle.gray(img)).cuda()) == q.contrast
        assert gq.compute_completeness(binary, c) == q.completeness


def test_blur_and_contrast_lower_scores(ctx):
    frames, corners, _ = synth_frames(1, 540, 960, seed=8, noise="int")
    img = frames.numpy()[0]
    binary = sv_oracle.preprocess_for_grid_detection(img)
    base = gq.assess_grid_quality(img, binary, corners[0])
    blurred = img
    for _ in range(3):
        blurred = np.stack([sv_oracle.gaussian_blur(blurred[..., c], 7) for c in range(3)], -1)
    assert gq.assess_grid_quality(blurred, binary, corners[0]).sharpness < base.sharpness
    flat = (img.astype(np.int32) // 4 + 96).astype(np.uint8)
    assert gq.assess_grid_quality(flat, binary, corners[0]).contrast < base.contrast


@pytest.mark.parametrize("bits_direct", [True, False])
def test_frame_pipeline_quality(ctx, bits_direct):
    ctx.load_state_dict(random_state_dict(1234))
    n, H, W = 64, 540, 960
    frames, _, _ = synth_frames(n, H, W, seed=17, device="cuda")
    frames = frames.contiguous()
    off = FramePipeline(ctx, H, W, chunk=16, depth=3, bits_direct=bits_direct).run(frames)
    p = FramePipeline(ctx, H, W, chunk=16, depth=3, bits_direct=bits_direct, quality=True)
    on = p.run(frames)
    again = p.run(frames)
    for k in ("digits", "logits", "conf"):
        assert torch.equal(off[k], on[k]), k
    assert (off["corners"] == on["corners"]).all() and (off["found"] == on["found"]).all()
    q = on["quality"]
    assert q.shape == (n, 6) and q.dtype == np.float32
    assert np.array_equal(q, again["quality"], equal_nan=True)
    binary = ctx.preprocess(frames)
    exp = gq.assess_grid_quality_batch(ctx, frames, binary, on["corners"], on["found"])
    assert np.array_equal(q, exp, equal_nan=True)
    for f in (0, 5, n - 1):
        if on["found"][f]:
            one = gq.assess_grid_quality(frames[f], binary[f], on["corners"][f])
            assert np.allclose(q[f], [one.overall, one.sharpness, one.contrast, one.completeness, one.geometry, one.size], rtol=0, atol=1e-3)
    assert not np.isnan(q[on["found"]]).any() and np.isnan(q[~on["found"]][:, [0, 3, 4, 5]]).all()


def test_frame_pipeline_quality_off_describe_unchanged(ctx):
    a = FramePipeline(ctx, 540, 960, chunk=16, depth=3)
    b = FramePipeline(ctx, 540, 960, chunk=16, depth=3, quality=True)
    assert a.describe() == b.describe() and not hasattr(a, "q_bin")


def test_recognize_image_quality(ctx, golden_dir):
    from sudoku_vision_amd.pipeline import recognize_image
    sd = random_state_dict(99)
    img = _photos(golden_dir)[0]
    base = recognize_image(img, sd, ctx=ctx)
    res = recognize_image(img, sd, ctx=ctx, quality=True)
    assert (res["digits"] == base["digits"]).all() and "quality" not in base
    binary = sv_oracle.preprocess_for_grid_detection(img)
    assert res["quality"] == gq.assess_grid_quality(img, binary, res["corners"])
    assert res["quality_feedback"] == gq.get_user_feedback(res["quality"])
