"""Counterpart of the reference's pipeline/overlay.py for the MI355X: the solved digits drawn into the camera frame itself, through
the homography of the detected corners (sv_render_overlay_u8, csrc/k16_overlay.hip) -- what the reference's roadmap calls the AR
overlay and its ios/.../SolutionOverlayView.swift does with an identity transform in place of the perspective one.

From pipeline/overlay.py come CellPrediction (:12-19), the 50-pixel cell (:27) and the three colours (:63-71).  Its two functions,
create_solution_overlay and create_debug_overlay, are not provided: they draw with cv2.putText, so every pixel of their output
depends on OpenCV's Hershey glyph tables, which are neither in the reference nor available to pin a restatement to; and they build
side-by-side composites with grid lines and labels, which is not what a camera feed shows.  The glyphs here are this project's own
stroke font (overlay_font.py); Context.set_overlay_glyphs takes any other 8-bit coverage atlas.  There is no CPU fallback.
"""
import os
import sys
from dataclasses import dataclass

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bootstrap import package  # noqa: E402
sys.path.pop(0)
_rt = package().runtime

CLASS_SOLVED, CLASS_ORIGINAL, CLASS_LOW_CONFIDENCE = 0, 1, 2      # rows of the default palette (pipeline/overlay.py:63-71)


@dataclass
class CellPrediction:
    """Prediction result for a single cell (pipeline/overlay.py:12-19)."""
    row: int
    col: int
    digit: int
    confidence: float
    is_original: bool = True


def overlay_cells(recognized_grid, solution, confidences=None, show_originals=False, low_confidence=0.7):
    """What to draw: -> (digits uint8 [81], classes uint8 [81]) for Context.render_overlay.
    Default, the iOS rule (SolutionOverlayView.swift:19-20): a cell is drawn only where the recognised digit is 0 and the solution
    is not, in class 0 (solved).  show_originals=True, pipeline/overlay.py:52-71: every non-zero cell of the solution is drawn; a cell
    that was recognised (non-zero in recognized_grid) is class 1 (original), or class 2 where confidences is given and its confidence
    is below low_confidence.  recognized_grid, solution: 9x9 or 81 values 0..9; confidences: 9x9 or 81 floats, or None."""
    rec = np.asarray(recognized_grid, np.int64).reshape(81)
    sol = np.asarray(solution, np.int64).reshape(81)
    if rec.min() < 0 or rec.max() > 9 or sol.min() < 0 or sol.max() > 9:
        raise ValueError("grids must hold values 0..9")
    original = rec != 0
    if not show_originals:
        return np.where(original, 0, sol).astype(np.uint8), np.zeros(81, np.uint8)
    classes = np.where(original, CLASS_ORIGINAL, CLASS_SOLVED)
    if confidences is not None:
        conf = np.asarray(confidences, np.float64).reshape(81)
        classes = np.where(original & (conf < low_confidence), CLASS_LOW_CONFIDENCE, classes)
    return sol.astype(np.uint8), classes.astype(np.uint8)


def cells_from_predictions(predictions, solution=None):
    """pipeline/overlay.py:52-71 from a list of CellPrediction: -> (digits uint8 [81], classes uint8 [81]); the digit is the
    solution's where one is given, else the prediction's; the class follows is_original and confidence < 0.7."""
    digits, classes = np.zeros(81, np.uint8), np.zeros(81, np.uint8)
    for p in predictions:
        x = 9 * p.row + p.col
        digits[x] = solution[p.row][p.col] if solution else p.digit
        classes[x] = (CLASS_LOW_CONFIDENCE if p.confidence < 0.7 else CLASS_ORIGINAL) if p.is_original else CLASS_SOLVED
    return digits, classes


def render_solution_on_frame(frame, corners, recognized_grid, solution, confidences=None, show_originals=False, low_confidence=0.7,
                             shadow=True, ctx=None):
    """One BGR frame (numpy uint8 [H,W,3] or a CUDA uint8 tensor of that shape) with the solution drawn at `corners` ([4,2], any
    order, as the corner search returns them) -> a new frame of the kind that was passed.  Corners that define no homography leave
    the frame unchanged (a copy)."""
    ctx = ctx or _rt.default_context()
    dev, was_tensor = _rt._to_dev(frame, ctx)
    if dev.dim() != 3 or dev.shape[2] != 3:
        raise ValueError(f"frame must have shape [H,W,3], got {list(dev.shape)}")
    digits, classes = overlay_cells(recognized_grid, solution, confidences, show_originals, low_confidence)
    m, ok = _rt.Context.corners_to_m_batch(np.asarray(corners, np.float32).reshape(1, 4, 2))
    out = ctx.render_overlay(dev[None], ctx.minv_to_device(m), torch.from_numpy(digits[None]).to(ctx.device),
                             torch.from_numpy(classes[None]).to(ctx.device), active=torch.from_numpy(ok.astype(np.uint8)).to(ctx.device),
                             shadow=shadow)
    return _rt._back(out[0], was_tensor)
