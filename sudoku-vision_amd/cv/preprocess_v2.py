"""MI355X drop-in for the reference's cv/preprocess_v2.py (same names, arguments, defaults, return types): what
pipeline/run_v2.py:278-280 does with a frame before anything else.

numpy uint8 in -> numpy uint8 out; a CUDA uint8 tensor in -> CUDA tensors out with no host round trip of an image.  All
pixel work runs in the HIP kernels of csrc/k7_preprocess_v2.hip (morphology, box mean, 21-tap Gaussian, division, CLAHE,
Sauvola, fixed thresholds and counts) and csrc/k1_threshold.hip (gray, 5-tap blur, adaptive threshold).  Only counts and
one 256-bin histogram cross to the host, where the decisions that need no pixels are taken:

    has_glare   count(gray > 250) / N > 0.01
    has_shadow  0.05 < count(gray - blur(gray, k) < -30) / N < 0.5,  k = max(H, W) // 20 made odd
    Otsu        OpenCV's double-precision pass over the histogram (otsu_from_histogram)
    strategy    per candidate 1 - |ratio - 0.1| / 0.1 for a white share in [0.02, 0.3], else 0; first maximum of
                adaptive, otsu, sauvola (choose_strategy)

There is no CPU fallback.  cv2 is not available to pin the arithmetic against; DESIGN.md section 2 states it.
"""
import os
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bootstrap import package  # noqa: E402
sys.path.pop(0)
_rt = package().runtime
_to_dev, _back = _rt._to_dev, _rt._back

METHODS = ("adaptive", "otsu", "sauvola")


@dataclass
class PreprocessResult:
    """Result of preprocessing with multiple outputs (cv/preprocess_v2.py:21-30)."""
    binary: np.ndarray
    gray: np.ndarray
    enhanced: np.ndarray
    illumination_normalized: Optional[np.ndarray] = None
    has_glare: bool = False
    has_shadow: bool = False
    method_used: str = "adaptive"


# ---- host side: everything that needs no pixels ---------------------------------------------------------------------------
def illumination_kernel_size(shape):
    """Side of normalize_illumination's ellipse for an image of `shape` (cv/preprocess_v2.py:47-50)."""
    k = max(shape[0], shape[1]) // 10
    if k % 2 == 0:
        k += 1
    return max(k, 51)


def shadow_kernel_size(shape):
    """Side of detect_shadow's box mean (cv/preprocess_v2.py:89-91)."""
    k = max(shape[0], shape[1]) // 20
    if k % 2 == 0:
        k += 1
    return k


def glare_flag(count, npx):
    """has_glare from the count of pixels above the threshold (cv/preprocess_v2.py:74-77)."""
    return bool(int(count) / int(npx) > 0.01)


def shadow_flag(count, npx):
    """has_shadow from the count of the shadow mask (cv/preprocess_v2.py:99-100)."""
    ratio = int(count) / int(npx)
    return bool(ratio > 0.05 and ratio < 0.5)


def otsu_from_histogram(hist):
    """cv2.threshold(..., THRESH_OTSU)'s threshold from the 256-bin histogram: OpenCV's single pass in double, in its
    operation order (oracle/sv_oracle.c svo_cell_ink_ratio states the same)."""
    h = [int(v) for v in np.asarray(hist).reshape(256)]
    total = sum(h)
    if total <= 0:
        raise ValueError("empty histogram")
    scale = 1.0 / float(total)
    mu = 0.0
    for i in range(256):
        mu += i * float(h[i])
    mu *= scale
    mu1 = q1 = max_sigma = 0.0
    max_val = 0
    eps = 1.1920928955078125e-07
    for i in range(256):
        p_i = h[i] * scale
        mu1 *= q1
        q1 += p_i
        q2 = 1.0 - q1
        if min(q1, q2) < eps or max(q1, q2) > 1.0 - eps:
            continue
        mu1 = (mu1 + i * p_i) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma, max_val = sigma, i
    return max_val


def score_binary_count(count, npx):
    """score_binary (cv/preprocess_v2.py:285-290) from the count of white pixels of a {0,255} image."""
    ratio = (255.0 * int(count) / int(npx)) / 255.0
    if ratio < 0.02 or ratio > 0.3:
        return 0
    return 1 - abs(ratio - 0.1) / 0.1


def choose_strategy(counts, npx):
    """Index into METHODS of the first best-scoring candidate (Python's max keeps the first maximum, :298)."""
    scores = [score_binary_count(c, npx) for c in counts]
    return max(range(len(scores)), key=lambda i: scores[i])


# ---- device plumbing ------------------------------------------------------------------------------------------------------
def _gray_planes(image, ctx, what):
    """A single-channel image -> (u8 [1,H,W] on device, was_tensor)."""
    d, was = _to_dev(image, ctx)
    if d.dim() != 2:
        raise ValueError(f"{what} expects a single-channel image")
    return d[None], was


def _grayscale_dev(d, ctx):
    """d u8 [H,W] or [H,W,3] on device -> gray u8 [1,H,W]."""
    if d.dim() == 2:
        return d[None]
    if d.dim() != 3 or d.shape[2] != 3:
        raise ValueError(f"expected an [H,W] or [H,W,3] image, got {list(d.shape)}")
    return ctx.gray(d[None])


def _normalize_illumination(ctx, g):
    background = ctx.morphology(g, ctx.MORPH_CLOSE, ctx.SHAPE_ELLIPSE, illumination_kernel_size(g.shape[1:]))
    return ctx.divide_normalize(g, background)


def _remove_shadow(ctx, g):
    background = ctx.gaussian_blur21(ctx.morphology(g, ctx.MORPH_DILATE, ctx.SHAPE_ELLIPSE, 7))
    return ctx.divide_normalize(g, background)


def _cleanup(ctx, b, close_size=3, open_size=2):
    if close_size > 0:
        b = ctx.morphology(b, ctx.MORPH_CLOSE, ctx.SHAPE_RECT, close_size)
    if open_size > 0:
        b = ctx.morphology(b, ctx.MORPH_OPEN, ctx.SHAPE_RECT, open_size)
    return b


def _conditions(ctx, g):
    """-> (has_glare, has_shadow, glare mask, shadow mask) with one device -> host copy of the two counts."""
    npx = g.shape[1] * g.shape[2]
    glare_mask, glare_n = ctx.threshold_count(g, 250)
    shadow_mask, shadow_n = ctx.shadow_mask(g, ctx.box_mean(g, shadow_kernel_size(g.shape[1:])))
    counts = torch.cat([glare_n, shadow_n]).cpu().numpy()
    return glare_flag(counts[0], npx), shadow_flag(counts[1], npx), glare_mask, shadow_mask


def _otsu_binary(ctx, g):
    hist = ctx.frame_quality_stats(g)[2][0].cpu().numpy()
    return ctx.threshold_count(g, otsu_from_histogram(hist), inv=True)[0]


# ---- the reference's names ------------------------------------------------------------------------------------------------
def grayscale(image):
    """Convert BGR image to grayscale (cv/preprocess_v2.py:33-37)."""
    if len(image.shape) == 2:
        return image  # already grayscale: the reference returns its argument
    ctx = _rt.default_context()
    d, was = _to_dev(image, ctx)
    return _back(_grayscale_dev(d, ctx)[0], was)


def normalize_illumination(gray):
    """Divide by the background estimated with a large elliptical closing (cv/preprocess_v2.py:40-60)."""
    ctx = _rt.default_context()
    g, was = _gray_planes(gray, ctx, "normalize_illumination")
    return _back(_normalize_illumination(ctx, g)[0], was)


def detect_glare(gray, threshold: int = 250):
    """-> (has_glare, glare mask u8 0/255): more than 1 % of the pixels above `threshold` (cv/preprocess_v2.py:63-79)."""
    ctx = _rt.default_context()
    g, was = _gray_planes(gray, ctx, "detect_glare")
    mask, n = ctx.threshold_count(g, int(threshold))
    return glare_flag(n.cpu().numpy()[0], g.shape[1] * g.shape[2]), _back(mask[0], was)


def detect_shadow(gray):
    """-> (has_shadow, shadow mask u8 0/255): pixels more than 30 below the local box mean (cv/preprocess_v2.py:82-102)."""
    ctx = _rt.default_context()
    g, was = _gray_planes(gray, ctx, "detect_shadow")
    mask, n = ctx.shadow_mask(g, ctx.box_mean(g, shadow_kernel_size(g.shape[1:])))
    return shadow_flag(n.cpu().numpy()[0], g.shape[1] * g.shape[2]), _back(mask[0], was)


def remove_shadow(gray):
    """Divide by the blurred 7x7 elliptical dilation (cv/preprocess_v2.py:105-119)."""
    ctx = _rt.default_context()
    g, was = _gray_planes(gray, ctx, "remove_shadow")
    return _back(_remove_shadow(ctx, g)[0], was)


def apply_clahe(gray, clip_limit: float = 2.0, tile_size: int = 8):
    """Contrast Limited Adaptive Histogram Equalization (cv/preprocess_v2.py:122-129)."""
    ctx = _rt.default_context()
    g, was = _gray_planes(gray, ctx, "apply_clahe")
    return _back(ctx.clahe(g, clip_limit, (tile_size, tile_size))[0], was)


def threshold_adaptive(gray, block_size: int = 11, c: int = 2):
    """Adaptive Gaussian threshold, inverted binary (cv/preprocess_v2.py:132-143)."""
    ctx = _rt.default_context()
    g, was = _gray_planes(gray, ctx, "threshold_adaptive")
    return _back(ctx.adaptive_threshold(g, block_size, c, inv=True)[0], was)


def threshold_otsu(gray):
    """Otsu's threshold, inverted binary (cv/preprocess_v2.py:146-149)."""
    ctx = _rt.default_context()
    g, was = _gray_planes(gray, ctx, "threshold_otsu")
    return _back(_otsu_binary(ctx, g)[0], was)


def threshold_sauvola(gray, window_size: int = 25, k: float = 0.2):
    """Sauvola's threshold T = mean * (1 + k * (std / 128 - 1)) (cv/preprocess_v2.py:152-175)."""
    ctx = _rt.default_context()
    g, was = _gray_planes(gray, ctx, "threshold_sauvola")
    return _back(ctx.threshold_sauvola(g, window_size, k)[0], was)


def morphological_cleanup(binary, close_size: int = 3, open_size: int = 2):
    """Rectangular close then open (cv/preprocess_v2.py:178-202)."""
    ctx = _rt.default_context()
    b, was = _gray_planes(binary, ctx, "morphological_cleanup")
    return _back(_cleanup(ctx, b, close_size, open_size)[0], was)


def preprocess_for_grid_detection(image, use_illumination_norm: bool = True, use_shadow_removal: bool = True):
    """Full preprocessing pipeline for grid detection (cv/preprocess_v2.py:205-244) -> binary, grid lines white."""
    ctx = _rt.default_context()
    d, was = _to_dev(image, ctx)
    g = _grayscale_dev(d, ctx)
    _, has_shadow, _, _ = _conditions(ctx, g)
    enhanced = g
    if has_shadow and use_shadow_removal:
        enhanced = _remove_shadow(ctx, enhanced)
    if use_illumination_norm:
        enhanced = _normalize_illumination(ctx, enhanced)
    enhanced = ctx.clahe(enhanced, 2.0, (8, 8))
    binary = ctx.adaptive_threshold(ctx.blur(enhanced, 5), 11, 2, inv=True)
    return _back(_cleanup(ctx, binary, 3, 2)[0], was)


def preprocess_multi_strategy(image):
    """Three thresholding strategies on the shadow-removed, illumination-normalised, CLAHE-enhanced image; the one whose
    share of white pixels is nearest 10 % wins (cv/preprocess_v2.py:247-308)."""
    ctx = _rt.default_context()
    d, was = _to_dev(image, ctx)
    g = _grayscale_dev(d, ctx)
    npx = g.shape[1] * g.shape[2]
    has_glare, has_shadow, _, _ = _conditions(ctx, g)
    normalized = _normalize_illumination(ctx, _remove_shadow(ctx, g) if has_shadow else g)
    enhanced = ctx.clahe(normalized, 2.0, (8, 8))
    blurred = ctx.blur(enhanced, 5)
    candidates = [_cleanup(ctx, ctx.adaptive_threshold(blurred, 11, 2, inv=True)),
                  None,
                  _cleanup(ctx, ctx.threshold_sauvola(blurred, 25, 0.2))]
    candidates[1] = _cleanup(ctx, _otsu_binary(ctx, blurred))
    counts = torch.cat([ctx.count_nonzero(b) for b in candidates]).cpu().numpy()
    best = choose_strategy(counts, npx)
    # without a shadow the image normalised on the way to `enhanced` is normalize_illumination(gray) itself
    illum = _normalize_illumination(ctx, g) if has_shadow else normalized
    gray_out = image if len(image.shape) == 2 else _back(g[0], was)
    return PreprocessResult(binary=_back(candidates[best][0], was), gray=gray_out, enhanced=_back(enhanced[0], was),
                            illumination_normalized=_back(illum[0], was), has_glare=has_glare, has_shadow=has_shadow,
                            method_used=METHODS[best])


def preprocess_cell(cell, clip_limit: float = 2.0, tile_size: int = 4):
    """CLAHE then adaptive threshold 11/2, white digit on black (cv/preprocess_v2.py:311-337), any cell size."""
    ctx = _rt.default_context()
    d, was = _to_dev(cell, ctx)
    g = _grayscale_dev(d, ctx)
    enhanced = ctx.clahe(g, clip_limit, (tile_size, tile_size))
    return _back(ctx.adaptive_threshold(enhanced, 11, 2, inv=False)[0], was)      # 255 - THRESH_BINARY_INV = THRESH_BINARY
