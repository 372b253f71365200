"""MI355X drop-in for the reference's cv/stabilizer.py (same names, arguments, defaults and return types): the temporal layer of a
camera feed, cv/stabilizer.py:308-335.

MotionDetector is the part with pixel work: gray, cv2.resize to 160x120, absdiff against the previous small frame, threshold, mean.
It runs as one launch of K15 (csrc/k15_motion.hip, Context.motion_update) that reads only the taps the resize needs; the previous
small frame stays on the device and one count per frame crosses to the host, where the reference's ratio comparison is made in
float64.  `update_batch` is an addition: n consecutive frames of the feed in one launch, identical to n `update` calls.

GridStabilizer is host bookkeeping over four corners and is plain numpy here.  cv2 is not a dependency of this package, so the eight
cv2.KalmanFilter(4, 2) objects are KalmanFilter below: float32, the same attribute names, the same predict() / correct() equations.

One behaviour of the reference is kept on purpose.  GridStabilizer.update never calls predict(), so a filter's errorCovPre stays zero,
correct() computes a zero gain, and statePost stays zero: with use_kalman=True (the default) the corners returned while fewer than
min_detections frames are in the history are EXACT ZEROS (raw_corners holds the detection).  From min_detections on the result is
the weighted mean of the history, which the filters do not touch.  A caller that calls _kalman_predict() itself gets ordinary Kalman
filters.

Importing this module creates no device context; GridStabilizer needs no GPU at all.
"""
import os
import sys
from collections import deque
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bootstrap import package  # noqa: E402
sys.path.pop(0)

SMALL_SIZE = (160, 120)          # (width, height) of the detector's small frame, cv/stabilizer.py:277


@dataclass
class StabilizedResult:
    """What GridStabilizer.update returns (cv/stabilizer.py:22-31)."""
    corners: Optional[np.ndarray]      # float32 [4,2], or None
    is_stable: bool                    # the history holds at least min_detections frames
    frames_detected: int               # frames in the history
    confidence: float                  # 0..1
    raw_corners: Optional[np.ndarray] = None   # the detection that was passed in


class KalmanFilter:
    """cv2.KalmanFilter(dynam_params, measure_params) without a control vector, CV_32F: the attributes and their initial values
    (transitionMatrix, processNoiseCov and measurementNoiseCov identity, everything else zero) and the two update steps."""

    def __init__(self, dynam_params=4, measure_params=2):
        n, m, f = dynam_params, measure_params, np.float32
        self.statePre, self.statePost = np.zeros((n, 1), f), np.zeros((n, 1), f)
        self.transitionMatrix, self.processNoiseCov = np.eye(n, dtype=f), np.eye(n, dtype=f)
        self.measurementMatrix, self.measurementNoiseCov = np.zeros((m, n), f), np.eye(m, dtype=f)
        self.errorCovPre, self.errorCovPost = np.zeros((n, n), f), np.zeros((n, n), f)
        self.gain = np.zeros((n, m), f)

    def predict(self):
        """x' = A x;  P' = A P A^T + Q;  both are also copied to the posterior, as cv2 does.  Returns statePre."""
        A = self.transitionMatrix
        self.statePre = (A @ self.statePost).astype(np.float32)
        self.errorCovPre = (A @ self.errorCovPost @ A.T + self.processNoiseCov).astype(np.float32)
        self.statePost, self.errorCovPost = self.statePre.copy(), self.errorCovPre.copy()
        return self.statePre

    def correct(self, measurement):
        """K = P' H^T (H P' H^T + R)^-1;  x = x' + K (z - H x');  P = P' - K H P'.  Returns statePost."""
        H = self.measurementMatrix
        hp = H @ self.errorCovPre                                        # H P'
        s = hp @ H.T + self.measurementNoiseCov
        self.gain = np.linalg.solve(s, hp).T.astype(np.float32)          # P' and s are symmetric: (s^-1 H P')^T = P' H^T s^-1
        z = np.asarray(measurement, np.float32).reshape(-1, 1)
        self.statePost = (self.statePre + self.gain @ (z - H @ self.statePre)).astype(np.float32)
        self.errorCovPost = (self.errorCovPre - self.gain @ hp).astype(np.float32)
        return self.statePost


class GridStabilizer:
    """Smooths the four detected corners over the last frames (cv/stabilizer.py:34-248).  See the module docstring for the zero
    corners that use_kalman=True yields before min_detections."""

    def __init__(self, buffer_size: int = 5, min_detections: int = 3, max_movement: float = 50.0, use_kalman: bool = True):
        self.buffer_size = buffer_size
        self.min_detections = min_detections
        self.max_movement = max_movement
        self.use_kalman = use_kalman
        self.corner_history: deque = deque(maxlen=buffer_size)
        self.last_stable_corners: Optional[np.ndarray] = None
        self.kalman_filters = self._new_filters() if use_kalman else None

    def _new_filters(self):
        return [self._create_kalman_filter() for _ in range(8)]           # corner i: filter 2i for x, 2i + 1 for y

    def _create_kalman_filter(self) -> KalmanFilter:
        """State (p, q, vp, vq) with constant velocity, measurement (p, q); Q = 0.01 I, R = I, P = I (cv/stabilizer.py:66-93)."""
        kf = KalmanFilter(4, 2)
        kf.transitionMatrix = np.eye(4, dtype=np.float32)
        kf.transitionMatrix[0, 2] = kf.transitionMatrix[1, 3] = 1
        kf.measurementMatrix = np.eye(2, 4, dtype=np.float32)
        kf.processNoiseCov = np.eye(4, dtype=np.float32) * 0.01
        kf.measurementNoiseCov = np.eye(2, dtype=np.float32)
        kf.errorCovPost = np.eye(4, dtype=np.float32)
        return kf

    def _is_valid_transition(self, new_corners, old_corners) -> bool:
        """No corner moved by more than max_movement (a move of exactly max_movement is accepted)."""
        if old_corners is None:
            return True
        return not any(np.linalg.norm(a - b) > self.max_movement for a, b in zip(new_corners, old_corners))

    def _average_corners(self, history: List[np.ndarray]):
        """Mean of the history with weights linspace(0.5, 1, len), newest heaviest, accumulated in float32."""
        if not history:
            return None
        weights = np.linspace(0.5, 1.0, len(history))
        weights = weights / weights.sum()
        mean = np.zeros((4, 2), np.float32)
        for w, corners in zip(weights, history):
            mean += w * corners
        return mean

    def _kalman_predict(self):
        """predict() on all eight filters -> the predicted corners float32 [4,2] (None without filters)."""
        if self.kalman_filters is None:
            return None
        out = np.zeros((4, 2), np.float32)
        for k, kf in enumerate(self.kalman_filters):
            out[k // 2, k % 2] = kf.predict()[0, 0]
        return out

    def _kalman_update(self, corners):
        """correct() on all eight filters with (coordinate, 0) -> their statePost[0] as float32 [4,2]."""
        if self.kalman_filters is None:
            return corners
        out = np.zeros((4, 2), np.float32)
        for k, kf in enumerate(self.kalman_filters):
            kf.correct(np.array([[corners[k // 2][k % 2]], [0]], np.float32))
            out[k // 2, k % 2] = kf.statePost[0, 0]
        return out

    def update(self, corners) -> StabilizedResult:
        """corners: this frame's detection, float32 [4,2], or None."""
        raw, history = corners, self.corner_history
        if corners is None:
            if history:
                history.popleft()                                          # a miss costs the oldest frame
            if self.last_stable_corners is not None and len(history) >= self.min_detections // 2:
                return StabilizedResult(self.last_stable_corners, False, len(history), len(history) / self.buffer_size * 0.5, raw)
            return StabilizedResult(None, False, len(history), 0, raw)
        if not self._is_valid_transition(corners, history[-1] if history else None):
            # an outlier is reported, not remembered
            return StabilizedResult(self.last_stable_corners, False, len(history), len(history) / self.buffer_size * 0.7, raw)
        history.append(corners.copy())
        if self.use_kalman:
            corners = self._kalman_update(corners)
        if len(history) >= self.min_detections:
            self.last_stable_corners = self._average_corners(list(history))
            return StabilizedResult(self.last_stable_corners, True, len(history), min(1.0, len(history) / self.buffer_size), raw)
        return StabilizedResult(corners, False, len(history), len(history) / self.buffer_size * 0.5, raw)

    def reset(self):
        self.corner_history.clear()
        self.last_stable_corners = None
        if self.use_kalman:
            self.kalman_filters = self._new_filters()


class MotionDetector:
    """The motion gate of cv/stabilizer.py:251-291 on the GPU.  `ctx` (an attribute): the Context to run on; None until the first
    frame, which takes the current device's default context."""

    def __init__(self, threshold: float = 30.0, min_area_ratio: float = 0.01):
        self.threshold = threshold
        self.min_area_ratio = min_area_ratio
        self.ctx = None
        self._prev = None                # u8 [120,160] on the device

    @property
    def prev_frame(self):
        """The previous small frame as numpy uint8 [120,160], None before the first frame.  Assigning None restarts the feed."""
        return None if self._prev is None else self._prev.cpu().numpy()

    @prev_frame.setter
    def prev_frame(self, value):
        if value is None:
            self._prev = None
        else:
            self._prev = package().runtime._to_dev(value, self._context())[0].contiguous()

    def _context(self):
        if self.ctx is None:
            self.ctx = package().runtime.default_context()
        return self.ctx

    def update_batch(self, frames) -> np.ndarray:
        """n consecutive frames of the feed, [n,H,W] gray or [n,H,W,3] BGR (numpy uint8 or a uint8 CUDA tensor) -> bool [n], what n
        update() calls would have returned; the state afterwards is theirs too."""
        ctx = self._context()
        dev, _ = package().runtime._to_dev(frames, ctx)
        if dev.dim() not in (3, 4):
            raise ValueError(f"frames must have shape [n,H,W] or [n,H,W,3], got {list(dev.shape)}")
        small, counts = ctx.motion_update(dev, self._prev, self.threshold, SMALL_SIZE)
        self._prev = small[-1] if len(small) == 1 else small[-1].clone()     # do not keep a whole batch alive for one frame
        ratio = counts.cpu().numpy().astype(np.float64) / float(SMALL_SIZE[0] * SMALL_SIZE[1])
        return ratio > self.min_area_ratio

    def update(self, frame) -> bool:
        """frame: gray [H,W] or BGR [H,W,3], numpy uint8 or a uint8 CUDA tensor -> True when more than min_area_ratio of the small
        frame's pixels differ from the previous small frame by more than threshold.  The first frame gives False."""
        if frame.ndim not in (2, 3):
            raise ValueError(f"frame must have shape [H,W] or [H,W,3], got {list(frame.shape)}")
        return bool(self.update_batch(frame[None])[0])
