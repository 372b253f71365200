"""MI355X drop-in for the reference's cv/grid_quality.py (same names, arguments, return types): the quality gate of
pipeline/run_v2.py:299-311.

The per-pixel work runs on the GPU as integer statistics (csrc/k6_quality.hip): the sum and the sum of squares of the
3x3 Laplacian, the 256-bin gray histogram, and per grid line band the count of warped binary pixels > 0.  The scores are
computed from them on the host:

    sharpness     var = (N*S2 - S1^2) / N^2 in Python integers, rounded once; min(100, var / 10)
    contrast      float32 cumsum of the histogram, left searchsorted of N*0.025 and N*0.975; min(100, range / 2)
    completeness  mean over the 20 bands of count / band pixels; min(100, mean / 0.5 * 100)
    geometry      side-length spread and corner angles of the ordered quad, float32 (corners only)
    size          average side / 9 against 15 / 30 px cells, float32 (corners only)
    overall       0.25 sharpness + 0.15 contrast + 0.25 completeness + 0.20 geometry + 0.15 size

Corners that do not define a homography (order_points picks one point twice for a quad rotated near 45 degrees, the
case sv_corners_to_minv_batch reports) get NaN for completeness, geometry, size and overall: the reference would warp
garbage there.  A NaN score raises no issue of its own; get_user_feedback then asks for a retake.
"""
import os
import sys
from dataclasses import dataclass, field
from typing import List

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bootstrap import package  # noqa: E402
sys.path.pop(0)
_rt = package().runtime

GRID_SIZE = 450
WEIGHTS = (0.25, 0.15, 0.25, 0.20, 0.15)          # sharpness, contrast, completeness, geometry, size
COLUMNS = ("overall", "sharpness", "contrast", "completeness", "geometry", "size")


def band_bounds(i):
    """Grid line i (0..9) -> [lo, hi) of its band across the 450-px warp (cv/grid_quality.py:116-134)."""
    c = min(i * (GRID_SIZE // 9), GRID_SIZE - 1)
    return max(0, c - 2), min(GRID_SIZE, c + 3)


# pixels per band in the order of sv_grid_line_coverage's counts: row line 0, column line 0, row line 1, ...
BAND_PIXELS = np.array([(hi - lo) * GRID_SIZE for i in range(10) for lo, hi in [band_bounds(i)] * 2], np.int64)


@dataclass
class QualityScore:
    """Quality assessment result (cv/grid_quality.py:22-45)."""
    overall: float
    sharpness: float
    contrast: float
    completeness: float
    geometry: float
    size: float
    issues: List[str] = field(default_factory=list)
    recommendations: List[str] = field(default_factory=list)

    @property
    def is_acceptable(self) -> bool:
        return self.overall >= 50

    @property
    def is_good(self) -> bool:
        return self.overall >= 70


# ---- host scoring from the integer statistics -----------------------------------------------------------------------
def laplacian_variance(lap_sum, lap_sqsum, npx):
    """Population variance of the Laplacian from its integer sums: one correctly rounded division of Python integers
    (N*S2 exceeds int64 for 10-MP photos)."""
    s1, s2, n = int(lap_sum), int(lap_sqsum), int(npx)
    return (n * s2 - s1 * s1) / (n * n)


def sharpness_from_stats(lap_sum, lap_sqsum, npx):
    return min(100.0, laplacian_variance(lap_sum, lap_sqsum, npx) / 10)


def contrast_indices(hist, npx):
    """(low, high) bins of the 2.5 % / 97.5 % points, with the reference's float32 cumulative histogram."""
    cum = np.cumsum(np.asarray(hist).reshape(256).astype(np.float32))
    return int(np.searchsorted(cum, npx * 0.025)), int(np.searchsorted(cum, npx * 0.975))


def contrast_from_hist(hist, npx):
    lo, hi = contrast_indices(hist, npx)
    return min(100.0, (hi - lo) / 2)


def completeness_from_counts(counts):
    """counts: the 20 band counts of one frame (sv_grid_line_coverage order)."""
    cover = np.asarray(counts, np.int64).reshape(20) / BAND_PIXELS
    return min(100.0, float(np.mean(cover)) / 0.5 * 100)


def _order_points(pts):
    """[n,4,2] -> top-left, top-right, bottom-right, bottom-left per quad, float32 (cv/grid.py:74-91 batched)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 4, 2)
    s = pts.sum(axis=2)
    d = pts[:, :, 1] - pts[:, :, 0]
    pick = np.stack([s.argmin(1), d.argmin(1), s.argmax(1), d.argmax(1)], 1)
    return np.take_along_axis(pts, pick[:, :, None], axis=1)


def _sides(o):
    e = np.roll(o, -1, axis=1) - o
    return np.sqrt((e * e).sum(axis=2))                      # [n,4] float32: |p[i+1] - p[i]|


def geometry_scores(corners):
    """compute_geometry for a batch of quads [n,4,2] -> float32 [n]."""
    o = _order_points(corners)
    sides = _sides(o)
    mean = sides.mean(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        variation = np.where(mean > 0, sides.std(axis=1) / mean, np.float32(1))
    p1, p2, p3 = o, np.roll(o, -1, axis=1), np.roll(o, -2, axis=1)
    v1, v2 = p1 - p2, p3 - p2
    norm = np.sqrt((v1 * v1).sum(axis=2)) * np.sqrt((v2 * v2).sum(axis=2)) + np.float32(1e-6)
    cos = (v1 * v2).sum(axis=2) / norm
    deviation = np.abs(np.degrees(np.arccos(np.clip(cos, np.float32(-1), np.float32(1)))) - np.float32(90)).mean(axis=1)
    side_score = np.maximum(np.float32(0), np.float32(100) - variation * np.float32(200))
    angle_score = np.maximum(np.float32(0), np.float32(100) - deviation * np.float32(5))
    return ((side_score + angle_score) / np.float32(2)).astype(np.float32)


def size_scores(corners):
    """compute_size_score for a batch of quads [n,4,2] -> float32 [n] (the image shape does not enter the score)."""
    cell = _sides(_order_points(corners)).mean(axis=1) / np.float32(9)
    small = cell / np.float32(15) * np.float32(30)
    mid = np.float32(30) + (cell - np.float32(15)) / np.float32(15) * np.float32(40)
    big = np.minimum(np.float32(100), np.float32(70) + (cell - np.float32(30)) / np.float32(20) * np.float32(30))
    return np.where(cell < 15, small, np.where(cell < 30, mid, big)).astype(np.float32)


def scores_from_stats(lap_sum, lap_sqsum, hist, counts, corners, ok, npx):
    """Host scoring of n frames from the GPU statistics -> float64 [n,6] (COLUMNS order).  corners [n,4,2]; ok [n] bool:
    found and non-degenerate (the four corner-dependent columns are NaN elsewhere); npx = H*W."""
    lap_sum, lap_sqsum = np.asarray(lap_sum).reshape(-1), np.asarray(lap_sqsum).reshape(-1)
    n = lap_sum.shape[0]
    hist, counts = np.asarray(hist).reshape(n, 256), np.asarray(counts).reshape(n, 20)
    ok = np.asarray(ok, bool).reshape(n)
    out = np.full((n, 6), np.nan)
    out[:, 1] = [sharpness_from_stats(lap_sum[f], lap_sqsum[f], npx) for f in range(n)]
    out[:, 2] = [contrast_from_hist(hist[f], npx) for f in range(n)]
    if ok.any():
        c = np.asarray(corners, np.float32).reshape(n, 4, 2)[ok]
        cover = (counts[ok].astype(np.int64) / BAND_PIXELS).mean(axis=1)
        out[ok, 3] = np.minimum(100.0, cover / 0.5 * 100)
        out[ok, 4] = geometry_scores(c)
        out[ok, 5] = size_scores(c)
        w = WEIGHTS
        out[ok, 0] = w[0] * out[ok, 1] + w[1] * out[ok, 2] + w[2] * out[ok, 3] + w[3] * out[ok, 4] + w[4] * out[ok, 5]
    return out


_CHECKS = ((1, 40, "Image is blurry", "Hold camera steady or improve focus"),
           (2, 40, "Low contrast", "Improve lighting conditions"),
           (3, 40, "Grid lines not fully visible", "Ensure entire puzzle is in frame"),
           (4, 50, "Grid is distorted", "Hold camera more perpendicular to puzzle"),
           (5, 40, "Puzzle appears too small", "Move camera closer to puzzle"))


def quality_score(row):
    """One row of scores_from_stats -> QualityScore with the reference's issues and recommendations (cv/grid_quality.py:251-270)."""
    row = [float(v) for v in row]
    issues, recs = [], []
    for col, limit, issue, rec in _CHECKS:
        if row[col] < limit:
            issues.append(issue)
            recs.append(rec)
    return QualityScore(*row, issues=issues, recommendations=recs)


def get_user_feedback(quality: QualityScore) -> str:
    """User-facing message (cv/grid_quality.py:284-300)."""
    if quality.is_good:
        return "Image quality is good. Processing..."
    if quality.is_acceptable:
        tip = f" Tip: {quality.recommendations[0]}" if quality.recommendations else ""
        return "Image quality is acceptable but could be better." + tip
    if quality.issues:
        return f"Please retake photo: {quality.issues[0]}. {quality.recommendations[0] if quality.recommendations else ''}"
    return "Image quality is too low. Please retake the photo."


# ---- the reference's functions, on the GPU --------------------------------------------------------------------------
def _host_corners(corners):
    c = corners.cpu().numpy() if isinstance(corners, torch.Tensor) else np.asarray(corners)
    return c.astype(np.float32).reshape(-1, 4, 2)


def _stats(image, ctx):
    """image [H,W] gray or [H,W,3] BGR -> (lap_sum, lap_sqsum, hist, H*W) on the host."""
    d, _ = _rt._to_dev(image, ctx)
    s1, s2, h = ctx.frame_quality_stats(d[None])
    return int(s1.item()), int(s2.item()), h[0].cpu().numpy(), d.shape[0] * d.shape[1]


def _coverage(binary, corners, ctx):
    """-> (counts int [20], ok) for one binary image and one quad."""
    minv, ok = _rt.Context.corners_to_minv_batch(_host_corners(corners), GRID_SIZE)
    counts = ctx.grid_line_coverage(_rt._to_dev(binary, ctx)[0][None], ctx.minv_to_device(minv))
    return counts[0].cpu().numpy(), bool(ok[0])


def compute_sharpness(gray) -> float:
    """Laplacian variance, 0-100 (cv/grid_quality.py:48-62)."""
    ctx = _rt.default_context()
    s1, s2, _, npx = _stats(gray, ctx)
    return sharpness_from_stats(s1, s2, npx)


def compute_contrast(gray) -> float:
    """95 % histogram spread, 0-100 (cv/grid_quality.py:65-87)."""
    ctx = _rt.default_context()
    _, _, hist, npx = _stats(gray, ctx)
    return contrast_from_hist(hist, npx)


def compute_completeness(binary, corners) -> float:
    """Ink share of the 20 grid line bands of the 450x450 warp, 0-100 (cv/grid_quality.py:90-149); NaN for degenerate corners."""
    counts, ok = _coverage(binary, corners, _rt.default_context())
    return completeness_from_counts(counts) if ok else float("nan")


def compute_geometry(corners) -> float:
    """Side-length consistency and corner angles, 0-100 (cv/grid_quality.py:152-193)."""
    return float(geometry_scores(_host_corners(corners))[0])


def compute_size_score(corners, image_shape=None) -> float:
    """Cell size, 0-100 (cv/grid_quality.py:196-219)."""
    return float(size_scores(_host_corners(corners))[0])


def assess_grid_quality(image, binary, corners, ctx=None) -> QualityScore:
    """All five metrics and the weighted overall score with the reference's feedback (cv/grid_quality.py:237-281).
    image: BGR [H,W,3] or gray [H,W]; binary [H,W] (preprocess_for_grid_detection); corners: 4 points, any order."""
    ctx = ctx or _rt.default_context()
    s1, s2, hist, npx = _stats(image, ctx)
    counts, ok = _coverage(binary, corners, ctx)
    return quality_score(scores_from_stats([s1], [s2], hist[None], counts[None], _host_corners(corners), [ok], npx)[0])


def assess_grid_quality_batch(ctx, frames, binary_or_bits, corners, ok):
    """n frames at once -> float32 [n,6] on the host (overall, sharpness, contrast, completeness, geometry, size).
    frames u8 [n,H,W,3] (or [n,H,W] gray) and binary_or_bits (u8 [n,H,W] or the bit image int32 [n,H,W//32]) on ctx's device;
    corners [n,4,2]; ok [n]: False where no grid was found -- those frames and degenerate quads get NaN in the four
    corner-dependent columns."""
    c = _host_corners(corners)
    minv, good = _rt.Context.corners_to_minv_batch(c, GRID_SIZE)
    good &= np.asarray(ok, bool).reshape(-1)
    s1, s2, hist = ctx.frame_quality_stats(frames)
    counts = ctx.grid_line_coverage(binary_or_bits, ctx.minv_to_device(minv))
    npx = frames.shape[1] * frames.shape[2]
    return scores_from_stats(s1.cpu().numpy(), s2.cpu().numpy(), hist.cpu().numpy(), counts.cpu().numpy(), c, good, npx).astype(np.float32)
