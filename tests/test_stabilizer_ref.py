"""CPU: tests/stabilizer_ref.py against the oracle's resize, the drop-in names of sudoku-vision_amd/cv/stabilizer.py, and
GridStabilizer (host numpy, no GPU) on scripted feeds."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import stabilizer_ref as R
import sv_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# coordinates below 4096 have a float32 half-ulp of at most 2.4e-4; the weighted mean takes at most six float32 roundings
TOL = 4e-3

SHAPES = [(1, 1), (5, 7), (119, 161), (120, 160), (240, 321), (241, 320), (251, 333), (1080, 1920)]


def _noise(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


@pytest.fixture(scope="module")
def S():
    import sudoku_vision_amd.cv.stabilizer as m
    return m


# ---- the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_small_frame_equals_oracle(shape):
    bgr = _noise(shape + (3,), sum(shape))
    assert (R.small_frame(bgr) == o.resize_linear(o.gray(bgr), (160, 120))).all()
    gray = _noise(shape, sum(shape) + 1)
    assert (R.small_frame(gray) == o.resize_linear(gray, (160, 120))).all()


def test_two_times_area_rule_by_hand():
    # sums 4k+1 (rounds down), 4k+2 (the tie, rounds up), 4k+3 (up), 4k (exact)
    img = np.array([[10, 11, 200, 201],
                    [12, 12, 202, 203],      # 45 -> 11 (11.25);    806 -> 201 (201.5 up to 202 -> (806+2)>>2 = 202)
                    [0, 1, 255, 255],
                    [1, 1, 255, 255]], np.uint8)    # 3 -> 1 (0.75 up); 1020 -> 255
    want = np.array([[(45 + 2) >> 2, (806 + 2) >> 2], [(3 + 2) >> 2, (1020 + 2) >> 2]], np.uint8)
    assert want.tolist() == [[11, 202], [1, 255]]
    assert (R.small_frame(img, (2, 2)) == want).all()
    assert (R.area2(img) == want).all()
    # one axis at 2x only is the linear table, which the oracle has
    for shape in ((4, 5), (5, 4)):
        x = _noise(shape, 9)
        assert (R.small_frame(x, (2, 2)) == o.resize_linear(x, (2, 2))).all()


def test_motion_counts_semantics():
    a = np.zeros((120, 160), np.uint8)
    b = a.copy()
    b[0, :5] = 31
    b[1, :7] = 30
    small, counts = R.motion_counts([a, b, b])
    assert (small[1] == b).all() and counts.tolist() == [0, 5, 0]
    assert R.motion_counts([b], prev_small=a, threshold=29.5)[1].tolist() == [12]
    d = R.Detector()
    assert [d.update(f) for f in (a, b, b)] == [False, False, False]


# ---- the drop-in's names ----------------------------------------------------------------------------------------------------
def test_stabilizer_dropin_names_resolve():
    """The reference's callers do sys.path.insert(cv/), `from stabilizer import ...`; importing creates no device context."""
    code = ("import sys; sys.path.insert(0, %r);"
            "from stabilizer import GridStabilizer, MotionDetector, StabilizedResult;"
            "import inspect;"
            "d = lambda f: [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[1:]];"
            "assert d(GridStabilizer.__init__) == [('buffer_size', 5), ('min_detections', 3), ('max_movement', 50.0), ('use_kalman', True)], d(GridStabilizer.__init__);"
            "assert d(MotionDetector.__init__) == [('threshold', 30.0), ('min_area_ratio', 0.01)], d(MotionDetector.__init__);"
            "assert [f for f in StabilizedResult.__dataclass_fields__] == ['corners', 'is_stable', 'frames_detected', 'confidence', 'raw_corners'];"
            "assert StabilizedResult(None, False, 0, 0.0).raw_corners is None;"
            "g = GridStabilizer(); m = MotionDetector();"
            "assert all(hasattr(g, n) for n in ('update', 'reset', '_is_valid_transition', '_average_corners', '_kalman_predict', '_kalman_update',"
            " 'corner_history', 'last_stable_corners', 'kalman_filters'));"
            "assert len(g.kalman_filters) == 8 and GridStabilizer(use_kalman=False).kalman_filters is None;"
            "assert m.prev_frame is None and m.threshold == 30.0 and m.min_area_ratio == 0.01 and hasattr(m, 'update_batch');"
            "sva = sys.modules.get('sudoku_vision_amd'); assert sva is None or not sva.runtime._default;"
            "print('ok')") % os.path.join(ROOT, "sudoku-vision_amd", "cv")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_signatures_of_the_methods(S):
    assert list(inspect.signature(S.GridStabilizer.update).parameters) == ["self", "corners"]
    assert list(inspect.signature(S.MotionDetector.update).parameters) == ["self", "frame"]
    assert list(inspect.signature(S.MotionDetector.update_batch).parameters) == ["self", "frames"]


# ---- GridStabilizer on scripted feeds ---------------------------------------------------------------------------------------
BASE = np.array([[100, 120], [900, 140], [880, 960], [90, 940]], np.float32)


def _feed(k):
    """Detection k of a steady feed: consecutive frames differ by 1 to 3 px per coordinate."""
    return BASE + np.float32(k) * np.array([[1, 2], [3, 1], [2, 2], [1, 3]], np.float32)


@pytest.mark.parametrize("use_kalman", [False, True])
def test_three_steady_detections_then_stable(S, use_kalman):
    g = S.GridStabilizer(use_kalman=use_kalman)
    seen = []
    for k in range(7):
        c = _feed(k)
        r = g.update(c)
        seen.append(c)
        assert r.raw_corners is c and r.frames_detected == min(k + 1, 5)
        if k < 2:
            assert not r.is_stable and r.confidence == (k + 1) / 5 * 0.5
            if use_kalman:
                assert r.corners.dtype == np.float32 and (r.corners == 0).all()       # the reference's never-predicted filters
            else:
                assert (r.corners == c).all()
        else:
            assert r.is_stable and r.confidence == min(1.0, min(k + 1, 5) / 5)
            want = R.weighted_mean(seen[-5:])
            assert r.corners.dtype == np.float32 and np.abs(r.corners - want).max() <= TOL
            assert r.corners is g.last_stable_corners
            # the weights run oldest -> newest: the reverse order is far off
            assert np.abs(R.weighted_mean(seen[-5:][::-1]) - want).max() > 0.1
    assert len(g.corner_history) == 5 and (g.corner_history[0] == _feed(2)).all()
    assert g.corner_history[-1] is not seen[-1]                                        # a copy is kept


@pytest.mark.parametrize("use_kalman", [False, True])
def test_jump_of_exactly_max_movement_and_just_over(S, use_kalman):
    g = S.GridStabilizer(use_kalman=use_kalman)
    for _ in range(3):
        stable = g.update(BASE.copy())
    assert stable.is_stable
    moved = BASE.copy()
    moved[2] += np.float32([30, 40])                    # a 3-4-5 triangle: exactly 50.0
    r = g.update(moved)
    assert r.is_stable and r.frames_detected == 4
    last = g.last_stable_corners.copy()
    far = moved.copy()
    far[0] += np.float32([30, 40.01])                   # just over 50 from the last accepted detection
    r = g.update(far)
    assert not r.is_stable and r.frames_detected == 4 and len(g.corner_history) == 4
    assert (r.corners == last).all() and r.raw_corners is far
    assert r.confidence == 4 / 5 * 0.7
    assert (g.corner_history[-1] == moved).all()        # the outlier was not remembered
    assert g._is_valid_transition(far, None) and g._is_valid_transition(moved, BASE) and not g._is_valid_transition(far, moved)


@pytest.mark.parametrize("use_kalman", [False, True])
def test_missed_detections_shrink_the_history(S, use_kalman):
    g = S.GridStabilizer(use_kalman=use_kalman)
    for k in range(4):
        g.update(_feed(k))
    last = g.last_stable_corners
    got = [g.update(None) for _ in range(5)]
    assert [r.frames_detected for r in got] == [3, 2, 1, 0, 0]
    # min_detections // 2 = 1: the last stable corners are handed out while one frame is left
    for r, left in zip(got[:3], (3, 2, 1)):
        assert r.corners is last and not r.is_stable and r.confidence == left / 5 * 0.5 and r.raw_corners is None
    for r in got[3:]:
        assert r.corners is None and r.confidence == 0 and not r.is_stable
    fresh = S.GridStabilizer(use_kalman=use_kalman)
    r = fresh.update(None)                              # nothing was ever stable
    assert r.corners is None and r.confidence == 0 and r.frames_detected == 0


def test_confidence_formulas_differ_where_tested(S):
    g = S.GridStabilizer(buffer_size=4, min_detections=3, use_kalman=False)
    assert g.update(_feed(0)).confidence == 1 / 4 * 0.5               # not enough detections: len / buffer * 0.5
    g.update(_feed(1))
    assert g.update(_feed(2)).confidence == 3 / 4                      # stable: min(1, len / buffer)
    assert g.update(_feed(2) + 500).confidence == 3 / 4 * 0.7          # outlier: len / buffer * 0.7
    assert g.update(None).confidence == 2 / 4 * 0.5                    # missed: len / buffer * 0.5
    for k in range(3, 9):
        r = g.update(_feed(k))
    assert r.confidence == 1.0 and r.frames_detected == 4


@pytest.mark.parametrize("use_kalman", [False, True])
def test_reset(S, use_kalman):
    g = S.GridStabilizer(use_kalman=use_kalman)
    for k in range(3):
        g.update(_feed(k))
    old = g.kalman_filters
    if use_kalman:
        g._kalman_predict()
    g.reset()
    assert len(g.corner_history) == 0 and g.last_stable_corners is None
    if use_kalman:
        assert g.kalman_filters is not old and len(g.kalman_filters) == 8
        assert (g.kalman_filters[0].errorCovPost == np.eye(4, dtype=np.float32)).all() and (g.kalman_filters[0].statePost == 0).all()
    else:
        assert g.kalman_filters is None
    r = g.update(_feed(0))
    assert not r.is_stable and r.frames_detected == 1


@pytest.mark.parametrize("use_kalman", [False, True])
def test_buffer_of_one(S, use_kalman):
    g = S.GridStabilizer(buffer_size=1, min_detections=1, use_kalman=use_kalman)
    for k in range(3):
        c = _feed(k)
        r = g.update(c)
        assert r.is_stable and r.frames_detected == 1 and r.confidence == 1.0
        assert np.abs(r.corners - c).max() <= TOL                                       # one frame, weight 1
    r = g.update(None)                                   # 0 >= 1 // 2: the last stable corners
    assert r.frames_detected == 0 and r.corners is g.last_stable_corners and r.confidence == 0.0


def test_kalman_attributes_and_never_predicted_state(S):
    g = S.GridStabilizer()
    kf = g.kalman_filters[3]
    for name, shape in (("transitionMatrix", (4, 4)), ("measurementMatrix", (2, 4)), ("processNoiseCov", (4, 4)), ("measurementNoiseCov", (2, 2)),
                        ("errorCovPost", (4, 4)), ("errorCovPre", (4, 4)), ("statePre", (4, 1)), ("statePost", (4, 1)), ("gain", (4, 2))):
        a = getattr(kf, name)
        assert a.dtype == np.float32 and a.shape == shape, name
    assert kf.transitionMatrix.tolist() == [[1, 0, 1, 0], [0, 1, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]]
    assert kf.measurementMatrix.tolist() == [[1, 0, 0, 0], [0, 1, 0, 0]]
    assert (kf.processNoiseCov == np.eye(4, dtype=np.float32) * np.float32(0.01)).all()
    c = _feed(0)
    out = g._kalman_update(c)
    assert out.dtype == np.float32 and (out == 0).all() and (kf.gain == 0).all() and (kf.statePost == 0).all()
    assert (S.GridStabilizer(use_kalman=False)._kalman_update(c) == c).all()
    assert S.GridStabilizer(use_kalman=False)._kalman_predict() is None


def test_kalman_after_predict_is_a_kalman_filter(S):
    """A constant measurement, predict then correct each round, against the float64 recursion of one coordinate's filter written out
    here: state (p, q, vp, vq), measurement (coordinate, 0)."""
    g = S.GridStabilizer()
    c = _feed(0)
    A = np.array([[1, 0, 1, 0], [0, 1, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    H = np.array([[1, 0, 0, 0], [0, 1, 0, 0]], np.float64)
    Q, Rm = np.eye(4) * 0.01, np.eye(2)
    x, P = np.zeros((8, 4, 1)), np.stack([np.eye(4)] * 8)
    rounds = 40
    for _ in range(rounds):
        pred = g._kalman_predict()
        got = g._kalman_update(c)
        for k in range(8):
            xp, Pp = A @ x[k], A @ P[k] @ A.T + Q
            K = Pp @ H.T @ np.linalg.inv(H @ Pp @ H.T + Rm)
            z = np.array([[float(c[k // 2, k % 2])], [0.0]])
            x[k], P[k] = xp + K @ (z - H @ xp), Pp - K @ H @ Pp
            assert abs(pred[k // 2, k % 2] - xp[0, 0]) <= 1e-3 * abs(z[0, 0])
        want = x[:, 0, 0].reshape(4, 2)
        assert np.abs(got - want).max() <= 1e-3 * np.abs(want).max() and (np.abs(got - want) <= 1e-3 * np.abs(c)).all()
    assert np.abs(got - c).max() <= 1e-3 * np.abs(c).max()                               # converged to the measurement
