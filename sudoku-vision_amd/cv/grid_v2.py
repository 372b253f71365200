"""MI355X drop-in for the reference's cv/grid_v2.py (same names, arguments, defaults, return types): the grid detection of
pipeline/run_v2.py:287, four methods tried in turn.

    contour          host corner search with run_v2's validity test (csrc/host_contours.cpp, sv_find_grid_corners_v2_u8)
    lines            cv2.HoughLinesP restated on the host (csrc/host_hough.cpp): sequential by construction
    contour_rotated  the Hough angle on the host, the full-frame cv2.warpAffine on the GPU (csrc/k13_grid_v2.hip), then contour
    harris_ransac    the full-frame cv2.goodFeaturesToTrack(useHarrisDetector=True) on the GPU (csrc/k13_grid_v2.hip), RANSAC on the host

Images are numpy uint8 arrays or uint8 CUDA tensors; the host stages read a tensor through one copy.  cv2.HoughLinesP seeds its
cv::RNG with a constant, so detect_lines is deterministic; fit_quadrilateral_ransac draws np.random.choice exactly where the
reference does, so a caller who seeds numpy sees the reference's sequence.
"""
import math
import os
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bootstrap import package  # noqa: E402
sys.path.pop(0)
_pkg = package()
_rt = _pkg.runtime
_host = _pkg.host


@dataclass
class GridDetectionResult:
    """Result of grid detection with metadata (cv/grid_v2.py:23-31)."""
    corners: Optional[np.ndarray]       # 4 corners float32, ordered; None if no grid was found
    confidence: float                   # 0.9 contour, 0.8 lines, 0.7 contour_rotated, 0.6 harris_ransac, 0 none
    method: str
    rotation_angle: float               # degrees; non-zero for contour_rotated only
    is_partial: bool
    debug_info: dict


def _on_host(img):
    return img.cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)


# ---- contour method -------------------------------------------------------------------------------------------------------
def find_contours(binary):
    """All external contours (cv/grid_v2.py:34-39)."""
    return _host.find_contours(_on_host(binary))


def approximate_polygon(contour, epsilon_ratio: float = 0.02):
    """cv2.approxPolyDP at epsilon_ratio * perimeter (cv/grid_v2.py:42-46)."""
    return _host.approx_poly_dp(contour, epsilon_ratio * _host.arc_length(contour, closed=True), closed=True)


def order_points(pts):
    """top-left, top-right, bottom-right, bottom-left as float32 (cv/grid_v2.py:49-61)."""
    pts = np.asarray(pts)
    total, delta = pts.sum(axis=1), np.diff(pts, axis=1).flatten()
    return np.stack([pts[np.argmin(total)], pts[np.argmin(delta)], pts[np.argmax(total)], pts[np.argmax(delta)]]).astype(np.float32)


def is_valid_quadrilateral(corners, min_angle: float = 45, max_angle: float = 135) -> bool:
    """Roughly rectangular: every angle in [min_angle, max_angle], longest side at most twice the shortest (cv/grid_v2.py:64-95)."""
    corners = np.asarray(corners)
    if corners.shape != (4, 2):
        return False
    nxt, after = np.roll(corners, -1, axis=0), np.roll(corners, -2, axis=0)
    for a, b in zip(corners - nxt, after - nxt):
        cos_angle = np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-6)
        angle = np.degrees(np.arccos(np.clip(cos_angle, -1, 1)))
        if angle < min_angle or angle > max_angle:
            return False
    sides = [np.linalg.norm(e) for e in nxt - corners]
    return not max(sides) > 2 * min(sides)


def detect_grid_contour(binary, min_area_ratio: float = 0.1):
    """The largest contour whose 4-vertex approximation is a valid quadrilateral, ordered, or None (cv/grid_v2.py:102-128)."""
    corners = _host.find_grid_corners_v2(_on_host(binary), min_area_ratio=min_area_ratio, epsilon_ratio=0.02)
    return None if corners is None else order_points(corners.astype(np.float32))


# ---- line method ----------------------------------------------------------------------------------------------------------
def detect_lines(binary, rho: float = 1, theta: float = np.pi / 180, threshold: int = 100, min_line_length: int = 50, max_line_gap: int = 10):
    """cv2.HoughLinesP -> int32 (N,1,4), or None when there is no line (cv/grid_v2.py:135-149)."""
    lines = _host.hough_lines_p(_on_host(binary), rho, theta, threshold, min_line_length, max_line_gap)
    return lines.reshape(-1, 1, 4) if len(lines) else None


def _direction(segment):
    x1, y1, x2, y2 = segment
    return np.degrees(np.arctan2(y2 - y1, x2 - x1))


def cluster_lines_by_angle(lines, angle_tolerance: float = 10):
    """-> (horizontal, vertical) lists of [x1,y1,x2,y2]; the rest is dropped (cv/grid_v2.py:152-172)."""
    horizontal, vertical = [], []
    for line in lines:
        angle = _direction(line[0]) % 180
        if abs(angle) < angle_tolerance or abs(angle - 180) < angle_tolerance:
            horizontal.append(line[0])
        elif abs(angle - 90) < angle_tolerance:
            vertical.append(line[0])
    return horizontal, vertical


def line_intersection(line1, line2):
    """Intersection of the two infinite lines, or None for parallel ones (cv/grid_v2.py:175-189)."""
    x1, y1, x2, y2 = line1
    x3, y3, x4, y4 = line2
    denom = (x1 - x2) * (y3 - y4) - (y1 - y2) * (x3 - x4)
    if abs(denom) < 1e-6:
        return None
    t = ((x1 - x3) * (y3 - y4) - (y1 - y3) * (x3 - x4)) / denom
    return (x1 + t * (x2 - x1), y1 + t * (y2 - y1))


def find_grid_from_lines(horizontal, vertical, image_shape):
    """The corners where the outermost horizontal and vertical lines meet (tl, tr, br, bl, float32), or None when there are fewer than
    two of either, two are parallel, or a corner lies more than 50 px outside the image (cv/grid_v2.py:192-234)."""
    if len(horizontal) < 2 or len(vertical) < 2:
        return None
    rows = sorted(horizontal, key=lambda s: (s[1] + s[3]) / 2)
    cols = sorted(vertical, key=lambda s: (s[0] + s[2]) / 2)
    met = [line_intersection(r, c) for r, c in ((rows[0], cols[0]), (rows[0], cols[-1]), (rows[-1], cols[-1]), (rows[-1], cols[0]))]
    if any(p is None for p in met):
        return None
    corners = np.array(met, dtype=np.float32)
    h, w = image_shape
    if any(x < -50 or x > w + 50 or y < -50 or y > h + 50 for x, y in corners):
        return None
    return corners


def detect_grid_lines(binary, min_area_ratio: float = 0.1):
    """Hough lines -> outermost horizontal / vertical pair -> corners, if they form a valid quadrilateral (cv/grid_v2.py:237-265)."""
    binary = _on_host(binary)
    h, w = binary.shape
    min_length = min(h, w) // 10
    lines = detect_lines(binary, threshold=50, min_line_length=min_length, max_line_gap=min_length // 5)
    if lines is None or len(lines) < 4:
        return None
    corners = find_grid_from_lines(*cluster_lines_by_angle(lines), (h, w))
    if corners is not None and is_valid_quadrilateral(corners):
        return order_points(corners)
    return None


# ---- corner method --------------------------------------------------------------------------------------------------------
def detect_corners_harris(gray, max_corners: int = 100, quality_level: float = 0.01, min_distance: int = 10):
    """cv2.goodFeaturesToTrack(useHarrisDetector=True) on the GPU -> float32 (N,2), or an empty array (cv/grid_v2.py:272-290)."""
    corners = _rt.default_context().harris_corners(gray, max_corners, quality_level, min_distance)
    if len(corners) == 0:
        return np.array([]) if not isinstance(corners, torch.Tensor) else corners
    return corners


def _shoelace(quad):
    """cv2.contourArea of float32 points: the shoelace sum in double."""
    q = np.asarray(quad, np.float32).astype(np.float64)
    p = np.roll(q, 1, axis=0)
    return abs(float(np.sum(p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0])) * 0.5)


def fit_quadrilateral_ransac(corners, image_shape, n_iterations: int = 100, inlier_threshold: float = 10):
    """The best of n_iterations random 4-subsets of corners: valid quadrilateral, at least 10 % of the image, score = half area share +
    half shortest/longest side (cv/grid_v2.py:293-339).  One np.random.choice per iteration, drawn before any test."""
    corners = _on_host(corners)
    if len(corners) < 4:
        return None
    h, w = image_shape
    best, best_score = None, 0
    for _ in range(n_iterations):
        quad = order_points(corners[np.random.choice(len(corners), 4, replace=False)])
        if not is_valid_quadrilateral(quad):
            continue
        share = _shoelace(quad) / (h * w)
        if share < 0.1:
            continue
        sides = [float(np.linalg.norm(e)) for e in np.roll(quad, -1, axis=0) - quad]      # float32 lengths, the score in double
        score = share * 0.5 + min(sides) / (max(sides) + 1e-6) * 0.5
        if score > best_score:
            best, best_score = quad, score
    return best


# ---- rotation -------------------------------------------------------------------------------------------------------------
def detect_rotation_angle(binary) -> float:
    """Median direction of the Hough lines, folded into (-45, 45] degrees; 0 with fewer than two lines (cv/grid_v2.py:346-368)."""
    lines = detect_lines(binary, threshold=30, min_line_length=30, max_line_gap=5)
    if lines is None or len(lines) < 2:
        return 0.0
    folded = [_direction(line[0]) % 90 for line in lines]
    return float(np.median([a - 90 if a > 45 else a for a in folded]))


def _rotation_matrix(center, angle):
    """cv2.getRotationMatrix2D(center, angle, 1.0)."""
    a = math.radians(angle)
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, s, (1 - c) * center[0] - s * center[1]], [-s, c, s * center[0] + (1 - c) * center[1]]], np.float64)


def rotate_image(image, angle: float):
    """Rotate about the centre into the enlarged bounding box, white border -> (rotated, forward 2x3 matrix) (cv/grid_v2.py:371-394)."""
    h, w = image.shape[:2]
    matrix = _rotation_matrix((w // 2, h // 2), angle)
    c, s = abs(matrix[0, 0]), abs(matrix[0, 1])
    new_w, new_h = int(h * s + w * c), int(h * c + w * s)
    matrix[0, 2] += (new_w - w) / 2
    matrix[1, 2] += (new_h - h) / 2
    return _rt.default_context().warp_affine(image, matrix, (new_w, new_h), 255), matrix


def _invert_affine(m):
    """cv2.invertAffineTransform of a 2x3 double matrix."""
    det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    det = 1.0 / det if det != 0 else 0.0
    a11, a22, a12, a21 = m[1, 1] * det, m[0, 0] * det, -m[0, 1] * det, -m[1, 0] * det
    return np.array([[a11, a12, -a11 * m[0, 2] - a12 * m[1, 2]], [a21, a22, -a21 * m[0, 2] - a22 * m[1, 2]]], np.float64)


# ---- the entry point ------------------------------------------------------------------------------------------------------
def detect_grid(binary, gray=None, try_rotation: bool = True, try_multiple_methods: bool = True) -> GridDetectionResult:
    """contour (0.9), lines (0.8), contour on the de-rotated image if the Hough angle exceeds 2 degrees (0.7), Harris corners +
    RANSAC when gray is given (0.6); method "none" with corners None otherwise (cv/grid_v2.py:401-508)."""
    binary_host = _on_host(binary)
    h, w = binary_host.shape
    debug_info = {}

    def found(corners, confidence, method, angle=0):
        return GridDetectionResult(corners=corners, confidence=confidence, method=method, rotation_angle=angle, is_partial=False, debug_info=debug_info)

    corners = detect_grid_contour(binary_host)
    if corners is not None:
        return found(corners, 0.9, "contour")
    if not try_multiple_methods:
        return found(None, 0, "none")

    corners = detect_grid_lines(binary_host)
    if corners is not None:
        return found(corners, 0.8, "lines")

    if try_rotation:
        rotation = detect_rotation_angle(binary_host)
        debug_info["detected_rotation"] = rotation
        if abs(rotation) > 2:
            rotated, matrix = rotate_image(binary, rotation)           # the caller's array or tensor: a tensor stays in HBM for the warp
            corners = detect_grid_contour(rotated)
            if corners is not None:
                back = (_invert_affine(matrix) @ np.hstack([corners, np.ones((4, 1))]).T).T.astype(np.float32)
                return found(back, 0.7, "contour_rotated", rotation)

    if gray is not None:
        harris = detect_corners_harris(gray)
        debug_info["harris_corners"] = len(harris)
        if len(harris) >= 4:
            corners = fit_quadrilateral_ransac(harris, (h, w))
            if corners is not None:
                return found(corners, 0.6, "harris_ransac")

    return found(None, 0, "none")


def warp_perspective(image, corners, output_size: int = 450):
    """Warp the grid region to an output_size square through K2's warp (cv/grid_v2.py:511-529)."""
    ctx = _rt.default_context()
    d, was_tensor = _rt._to_dev(image, ctx)
    quad = np.asarray(corners.cpu() if isinstance(corners, torch.Tensor) else corners).astype(np.float32).reshape(1, 4, 2)
    minv = ctx.minv_to_device(_rt.Context.corners_to_minv(quad, output_size, 0.0))
    return _rt._back(ctx.warp_perspective(d, minv, output_size), was_tensor)
