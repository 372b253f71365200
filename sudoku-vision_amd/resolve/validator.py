"""Drop-in for the reference's pipeline/validator.py: the names, fields, argument names and defaults that pipeline/run_v2.py:42 imports,
with the validation itself on the MI355X (sv_resolve_conflicts, csrc/k9_resolve.hip).  Put this directory ahead of the reference's
pipeline/ on sys.path; constraint_resolver is then this directory's too (csrc/k10_propagate.hip).

validate_predictions asks the device for the number of conflicts and for how many conflicts name each cell, and lists the Conflict
objects (which are text) on the host from the same digits; the two are checked against each other.

Confidences are rounded to float32 on the way in, because that is what the device holds.  run_v2 only ever passes float32 softmax
outputs (pipeline/run_v2.py:166-188), for which this changes nothing.  A cell may carry at most 3 alternatives (ValueError otherwise).
There is no CPU fallback.
"""
import os
import sys
from dataclasses import dataclass, field
from typing import List, Set, Tuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bootstrap import package  # noqa: E402
sys.path.pop(0)
_rt = package().runtime

MAX_ALTERNATIVES = 3
_NONE = 255                       # an alternative slot that holds nothing (include/sudoku_vision_hip.h, sv_resolve_conflicts)


@dataclass
class Conflict:
    """A digit that a row, a column or a box shows more than once."""
    type: str                     # 'row', 'column', 'box'
    digit: int
    cells: List[Tuple[int, int]]
    description: str


@dataclass
class CellInfo:
    """What the recogniser says about one cell."""
    row: int
    col: int
    digit: int                    # 0 = empty
    confidence: float = 1.0
    alternatives: List[Tuple[int, float]] = field(default_factory=list)


@dataclass
class ValidationResult:
    is_valid: bool
    conflicts: List[Conflict]
    cells_in_conflict: Set[Tuple[int, int]]
    num_conflicts: int = 0
    num_cells_affected: int = 0

    def __post_init__(self):
        self.num_conflicts = len(self.conflicts)
        self.num_cells_affected = len(self.cells_in_conflict)


def get_box_index(row: int, col: int) -> int:
    return 3 * (row // 3) + col // 3


def get_box_cells(box_index: int) -> List[Tuple[int, int]]:
    top, left = 3 * (box_index // 3), 3 * (box_index % 3)
    return [(top + i, left + j) for i in range(3) for j in range(3)]


def cells_to_arrays(cells):
    """81 CellInfo in any order -> (index u8 [1,81,k], prob f32 [1,81,k]) laid out by (row, col), k = 1 + the most alternatives of a cell."""
    if len(cells) != 81 or {(c.row, c.col) for c in cells} != {(r, c) for r in range(9) for c in range(9)}:
        raise ValueError("expected the 81 cells of a 9x9 grid")
    most = max(len(c.alternatives) for c in cells)
    if most > MAX_ALTERNATIVES:
        raise ValueError(f"a cell has {most} alternatives; the device search takes at most {MAX_ALTERNATIVES}")
    index = np.full((1, 81, 1 + most), _NONE, np.uint8)
    prob = np.zeros((1, 81, 1 + most), np.float32)
    for c in cells:
        x = 9 * c.row + c.col
        index[0, x, 0], prob[0, x, 0] = c.digit, c.confidence
        for j, (d, p) in enumerate(c.alternatives):
            index[0, x, 1 + j], prob[0, x, 1 + j] = d, p
    return index, prob


def device_resolve(cells, beam_width, max_corrections, min_alternative_confidence):
    """The cells through Context.resolve_conflicts on the current device -> its outputs for the one frame, as host arrays."""
    ctx = _rt.default_context()
    index, prob = cells_to_arrays(cells)
    out = ctx.resolve_conflicts(torch.from_numpy(index).to(ctx.device), torch.from_numpy(prob).to(ctx.device), beam_width, max_corrections,
                                min_alternative_confidence)
    return {k: v[0].cpu().numpy() for k, v in out.items()}


def validation_from(digits, num_conflicts, conflict_count):
    """The device's verdict on 81 digits as a ValidationResult: conflicts by rows, then columns, then boxes, digits in order of
    first appearance, with the reference's description strings."""
    units = [("row", r, [(r, c) for c in range(9)]) for r in range(9)] + [("column", c, [(r, c) for r in range(9)]) for c in range(9)] + \
            [("box", b, get_box_cells(b)) for b in range(9)]
    conflicts, named = [], {}
    for kind, u, members in units:
        seen = {}
        for r, c in members:
            d = int(digits[9 * r + c])
            if d > 0:
                seen.setdefault(d, []).append((r, c))
        for d, where in seen.items():
            if len(where) > 1:
                if kind == "row":
                    text = f"Row {u + 1}: digit {d} appears at columns {[c + 1 for _, c in where]}"
                elif kind == "column":
                    text = f"Column {u + 1}: digit {d} appears at rows {[r + 1 for r, _ in where]}"
                else:
                    text = f"Box {u + 1}: digit {d} appears {len(where)} times"
                conflicts.append(Conflict(type=kind, digit=d, cells=where, description=text))
                for rc in where:
                    named[rc] = named.get(rc, 0) + 1
    if len(conflicts) != int(num_conflicts) or any(named.get((x // 9, x % 9), 0) != int(conflict_count[x]) for x in range(81)):
        raise RuntimeError("the device's validation and the host's conflict list disagree")
    return ValidationResult(is_valid=not conflicts, conflicts=conflicts, cells_in_conflict=set(named))


def validate_predictions(cells: List[CellInfo]) -> ValidationResult:
    """The sudoku rules on 81 predictions (pipeline/run_v2.py:347)."""
    out = device_resolve(cells, 1, 0, 0.1)
    return validation_from(out["digits"], out["num_conflicts_before"], out["conflict_count"])
