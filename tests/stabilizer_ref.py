"""A numpy restatement of MotionDetector (the reference's cv/stabilizer.py:251-291) for the tests of csrc/k15_motion.hip and
sudoku-vision_amd/cv/stabilizer.py, built from warp_ref.bgr_to_gray and warp_ref.resize plus the one case those do not have:

  * a source that already has the target size is copied (warp_ref.resize does that);
  * a source of exactly twice the target on BOTH axes is not interpolated: cv2.resize turns INTER_LINEAR into INTER_AREA there
    (OpenCV's resize.cpp, where the integer scale factors of an exact integer reduction are both 2), and the 8-bit 2x2 area path is (s00 + s01 + s10 + s11 + 2) >> 2.  One axis at exactly 2x is still linear.  Taken from OpenCV's source: cv2 is not
    installed where this project is developed, so the rule has not been run against cv2.

GridStabilizer is restated only as the weighted mean its stable output is, in float64 (the rest of its expectations are written out
by hand in tests/test_stabilizer_ref.py).
"""
import numpy as np

import warp_ref

SMALL = (160, 120)             # (dw, dh)


def area2(gray):
    """The 2x2 mean of a gray image with even sides, rounded half up."""
    g = np.asarray(gray, np.int64)
    return ((g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def small_frame(frame, dsize=SMALL):
    """frame u8 [H,W] or [H,W,3] (BGR) -> cv2.resize(gray(frame), dsize), dsize = (dw, dh)."""
    frame = np.asarray(frame, np.uint8)
    gray = warp_ref.bgr_to_gray(frame) if frame.ndim == 3 else frame
    dw, dh = dsize
    if gray.shape == (2 * dh, 2 * dw):
        return area2(gray)
    return warp_ref.resize(gray, (dw, dh))


def motion_counts(frames, prev_small=None, threshold=30.0, dsize=SMALL):
    """-> (small u8 [n,dh,dw], counts int64 [n]): per frame the small image and the pixels whose difference from the previous small
    image is > threshold, compared as numpy compares an integer array with a Python float; counts[0] = 0 without prev_small."""
    small = np.stack([small_frame(f, dsize) for f in frames])
    counts = np.zeros(len(small), np.int64)
    prev = prev_small
    for i, s in enumerate(small):
        if prev is not None:
            diff = np.abs(s.astype(np.int64) - np.asarray(prev, np.int64))
            counts[i] = int((diff.astype(np.float64) > float(threshold)).sum())
        prev = s
    return small, counts


class Detector:
    """MotionDetector.update, frame by frame."""

    def __init__(self, threshold=30.0, min_area_ratio=0.01):
        self.threshold, self.min_area_ratio, self.prev_frame = threshold, min_area_ratio, None

    def update(self, frame):
        small, counts = motion_counts([frame], self.prev_frame, self.threshold)
        self.prev_frame = small[0]
        return bool(np.float64(counts[0]) / np.float64(small[0].size) > self.min_area_ratio)


def weighted_mean(history):
    """GridStabilizer's stable corners: the mean of the history with weights linspace(0.5, 1, len), in float64."""
    w = np.linspace(0.5, 1.0, len(history))
    w = w / w.sum()
    return sum(wi * np.asarray(c, np.float64) for wi, c in zip(w, history))
