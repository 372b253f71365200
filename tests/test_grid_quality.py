"""CPU (-m "not gpu"): the quality gate's host scoring (sudoku_vision_amd.cv.grid_quality) fed with integer statistics computed
by numpy from oracle images, against the reference's formulas restated in float64 (quality_ref.py): synthetic frames and the
five sample photos."""
import os

import numpy as np
import pytest

import quality_ref as R
import sv_oracle
from sudoku_vision_amd import host
from sudoku_vision_amd.cv import grid_quality as gq
from sudoku_vision_amd.synth import synth_frames


def _score(img, binary, corners, ok=True):
    s1, s2, hist, gray = R.frame_stats(img)
    counts = R.coverage_counts(binary, corners) if ok else np.zeros(20, np.int64)
    row = gq.scores_from_stats([s1], [s2], hist[None], counts[None], np.asarray(corners, np.float32)[None], [ok], gray.size)[0]
    return gq.quality_score(row), (s1, s2, hist, gray)


def _check_frame(img, binary, corners):
    q, (s1, s2, hist, gray) = _score(img, binary, corners)
    var = gq.laplacian_variance(s1, s2, gray.size)
    ref_var = R.ref_sharpness(gray)[1]
    assert abs(var - ref_var) <= 1e-10 * abs(ref_var)
    assert gq.contrast_indices(hist, gray.size) == R.ref_contrast(gray)[1]
    r = R.ref_assess(img, binary, corners)
    R.compare(q, r)
    if not R.near_threshold(r):
        assert gq.get_user_feedback(q) == r["feedback"]
    return q


@pytest.fixture(scope="module")
def synth():
    frames, corners, _ = synth_frames(4, 270, 480, seed=5, noise="int")
    return frames.numpy(), corners


def test_band_geometry():
    assert gq.BAND_PIXELS.sum() == 41400
    assert [gq.band_bounds(i) for i in (0, 1, 9)] == [(0, 3), (48, 53), (447, 450)]


def test_synthetic_frames(synth):
    frames, corners = synth
    for f in range(frames.shape[0]):
        binary = sv_oracle.preprocess_for_grid_detection(frames[f])
        _check_frame(frames[f], binary, corners[f])


def test_degraded_frames_score_lower(synth):
    frames, corners = synth
    img = frames[0]
    binary = sv_oracle.preprocess_for_grid_detection(img)
    base = _check_frame(img, binary, corners[0])
    blurred = np.stack([sv_oracle.gaussian_blur(img[..., c], 7) for c in range(3)], -1)
    blurred = np.stack([sv_oracle.gaussian_blur(blurred[..., c], 7) for c in range(3)], -1)
    assert _check_frame(blurred, binary, corners[0]).sharpness < base.sharpness
    flat = (img.astype(np.int32) // 4 + 96).astype(np.uint8)
    assert _check_frame(flat, binary, corners[0]).contrast < base.contrast


def test_gray_input(synth):
    frames, corners = synth
    gray = sv_oracle.gray(frames[1])
    _check_frame(gray, sv_oracle.preprocess_for_grid_detection(frames[1]), corners[1])


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_sample_photos(golden_dir, k):
    with open(os.path.join(golden_dir, f"sample_{k}.jpg"), "rb") as fh:
        img = sv_oracle.imdecode(fh.read())
    binary = sv_oracle.preprocess_for_grid_detection(img)
    corners = host.find_grid_corners(binary)
    if corners is None:      # no grid: only the frame statistics are defined
        q, (s1, s2, hist, gray) = _score(img, binary, np.zeros((4, 2), np.float32), ok=False)
        assert abs(q.sharpness - R.ref_sharpness(gray)[0]) <= 1e-3
        assert gq.contrast_indices(hist, gray.size) == R.ref_contrast(gray)[1]
        assert np.isnan(q.overall) and np.isnan(q.completeness)
        return
    _check_frame(img, binary, corners.astype(np.float32))


def test_degenerate_corners_are_nan(synth):
    frames, corners = synth
    # a square rotated by 45 degrees: order_points picks one vertex twice
    diamond = np.array([[240, 35], [340, 135], [240, 235], [140, 135]], np.float32)
    minv, ok = gq._rt.Context.corners_to_minv_batch(diamond[None], 450)
    assert not ok[0]
    s1, s2, hist, gray = R.frame_stats(frames[0])
    rows = gq.scores_from_stats([s1, s1], [s2, s2], np.stack([hist, hist]), np.zeros((2, 20), np.int64),
                                np.stack([diamond, corners[0]]), [False, True], gray.size)
    assert np.isnan(rows[0, [0, 3, 4, 5]]).all() and np.isfinite(rows[0, 1:3]).all()
    assert np.isfinite(rows[1]).all()
    q = gq.quality_score(rows[0])
    assert not q.is_acceptable and gq.get_user_feedback(q).startswith(("Please retake photo", "Image quality is too low"))


def test_variance_exact_beyond_int64():
    # 10-MP frame: N*S2 overflows int64, the Python-integer formula does not
    n, s1, s2 = 10_000_000, 123_456_789, 9_000_000_000_000
    assert n * s2 > 2 ** 63
    assert gq.laplacian_variance(s1, s2, n) == (n * s2 - s1 * s1) / (n * n)
