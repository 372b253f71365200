"""Test helpers for the quality gate (cv/grid_quality.py): the integer statistics computed with numpy from oracle images,
and the reference's scoring formulas restated independently in float64 numpy -- the yardstick for
sudoku_vision_amd.cv.grid_quality's host scoring and for the K6 kernels."""
import numpy as np

import sv_oracle

BAND_HALF = 2          # a band is the line's pixel row/column +-2
SIZE = 450


def laplacian(gray):
    """cv2.Laplacian(gray, CV_64F) with ksize 1: [0 1 0; 1 -4 1; 0 1 0], BORDER_REFLECT_101 (np.pad 'reflect'); a 1-pixel axis
    is its own neighbour."""
    g = np.asarray(gray, np.int64)
    modes = ["reflect" if n > 1 else "edge" for n in g.shape]
    p = np.pad(g, ((1, 1), (0, 0)), mode=modes[0])
    p = np.pad(p, ((0, 0), (1, 1)), mode=modes[1])
    return p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4 * g


def frame_stats(img):
    """img BGR [H,W,3] or gray [H,W] -> (lap_sum, lap_sqsum, hist int64 [256], gray)."""
    gray = sv_oracle.gray(img) if img.ndim == 3 else np.asarray(img, np.uint8)
    lap = laplacian(gray)
    return int(lap.sum()), int((lap * lap).sum()), np.bincount(gray.ravel(), minlength=256), gray


def band_slices(i):
    c = min(i * (SIZE // 9), SIZE - 1)
    return slice(max(0, c - BAND_HALF), min(SIZE, c + BAND_HALF + 1))


def warped_counts(warped):
    """counts[20] of pixels > 0 per band (row line i, column line i, ...) of a 450x450 warp."""
    out = []
    for i in range(10):
        sl = band_slices(i)
        out += [int((warped[sl, :] > 0).sum()), int((warped[:, sl] > 0).sum())]
    return np.array(out, np.int64)


def coverage_counts(binary, corners):
    return warped_counts(sv_oracle.warp_perspective(binary, corners, SIZE))


# ---- the reference's formulas, written out in float64 numpy ----------------------------------------------------------
def ref_sharpness(gray):
    var = float(np.var(laplacian(gray).astype(np.float64)))
    return min(100, var / 10), var


def ref_contrast(gray):
    hist = np.bincount(gray.ravel(), minlength=256).astype(np.float32).reshape(256, 1)   # calcHist's dtype and shape
    cum = np.cumsum(hist)
    lo, hi = np.searchsorted(cum, gray.size * 0.025), np.searchsorted(cum, gray.size * 0.975)
    return min(100, (hi - lo) / 2), (int(lo), int(hi))


def ref_completeness(warped):
    scores = []
    for i in range(10):
        sl = band_slices(i)
        scores.append(np.mean(warped[sl, :] > 0))
        scores.append(np.mean(warped[:, sl] > 0))
    return min(100, np.mean(scores) / 0.5 * 100)


def _ordered(corners):
    return sv_oracle.order_points(np.asarray(corners, np.float32).reshape(4, 2)).astype(np.float64)


def ref_geometry(corners):
    q = _ordered(corners)
    sides = [np.hypot(*(q[(k + 1) % 4] - q[k])) for k in range(4)]
    m = np.mean(sides)
    var = np.std(sides) / m if m > 0 else 1
    dev = []
    for k in range(4):
        a, b, c = q[k], q[(k + 1) % 4], q[(k + 2) % 4]
        u, v = a - b, c - b
        cosv = np.dot(u, v) / (np.hypot(*u) * np.hypot(*v) + 1e-6)
        dev.append(abs(np.degrees(np.arccos(np.clip(cosv, -1, 1))) - 90))
    return (max(0, 100 - var * 200) + max(0, 100 - np.mean(dev) * 5)) / 2


def ref_size(corners):
    q = _ordered(corners)
    cell = np.mean([np.hypot(*(q[(k + 1) % 4] - q[k])) for k in range(4)]) / 9
    if cell < 15:
        return cell / 15 * 30
    if cell < 30:
        return 30 + (cell - 15) / 15 * 40
    return min(100, 70 + (cell - 30) / 20 * 30)


THRESHOLDS = {"sharpness": 40, "contrast": 40, "completeness": 40, "geometry": 50, "size": 40}
MESSAGES = {"sharpness": ("Image is blurry", "Hold camera steady or improve focus"),
            "contrast": ("Low contrast", "Improve lighting conditions"),
            "completeness": ("Grid lines not fully visible", "Ensure entire puzzle is in frame"),
            "geometry": ("Grid is distorted", "Hold camera more perpendicular to puzzle"),
            "size": ("Puzzle appears too small", "Move camera closer to puzzle")}


def ref_assess(image, binary, corners):
    """-> dict of the five scores, overall, issues, recommendations, feedback."""
    gray = sv_oracle.gray(image) if image.ndim == 3 else image
    r = {"sharpness": ref_sharpness(gray)[0], "contrast": ref_contrast(gray)[0],
         "completeness": ref_completeness(sv_oracle.warp_perspective(binary, corners, SIZE)),
         "geometry": ref_geometry(corners), "size": ref_size(corners)}
    r["overall"] = (0.25 * r["sharpness"] + 0.15 * r["contrast"] + 0.25 * r["completeness"] + 0.20 * r["geometry"]
                    + 0.15 * r["size"])
    r["issues"] = [MESSAGES[k][0] for k in THRESHOLDS if r[k] < THRESHOLDS[k]]
    r["recommendations"] = [MESSAGES[k][1] for k in THRESHOLDS if r[k] < THRESHOLDS[k]]
    if r["overall"] >= 70:
        r["feedback"] = "Image quality is good. Processing..."
    elif r["overall"] >= 50:
        r["feedback"] = "Image quality is acceptable but could be better." + (f" Tip: {r['recommendations'][0]}" if r["recommendations"] else "")
    elif r["issues"]:
        r["feedback"] = f"Please retake photo: {r['issues'][0]}. {r['recommendations'][0]}"
    else:
        r["feedback"] = "Image quality is too low. Please retake the photo."
    return r


def near_threshold(r, tol=1e-3):
    """True when a score lies within tol of a threshold its feedback depends on (then strings may legitimately differ)."""
    if any(abs(r[k] - THRESHOLDS[k]) <= tol for k in THRESHOLDS):
        return True
    return abs(r["overall"] - 70) <= tol or abs(r["overall"] - 50) <= tol


def compare(q, r, tol=1e-3):
    """q: a QualityScore; r: ref_assess's dict.  Asserts the tolerances of the quality gate's tests."""
    for k in ("overall", "sharpness", "contrast", "completeness", "geometry", "size"):
        assert abs(getattr(q, k) - r[k]) <= tol, (k, getattr(q, k), r[k])
    if not near_threshold(r, tol):
        assert q.issues == r["issues"] and q.recommendations == r["recommendations"], (q, r)
