"""Drop-in for the reference's pipeline/conflict_resolver.py: the names, fields, argument names and defaults that pipeline/run_v2.py:43
imports, with the beam search itself on the MI355X (sv_resolve_conflicts, csrc/k9_resolve.hip): one launch per call, every field of
the result equal to the reference's, the score to the bit.

Confidences are rounded to float32 on the way in; run_v2 only ever passes float32 softmax outputs, for which this changes nothing.
A cell may carry at most 3 alternatives, beam_width is 1..6 and max_corrections 0..3 (the library refuses anything else).
There is no CPU fallback.
"""
import os
import sys
from dataclasses import dataclass
from typing import List

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from validator import CellInfo, ValidationResult, device_resolve, validation_from, _NONE  # noqa: E402
sys.path.pop(0)


@dataclass
class CorrectionCandidate:
    """One cell given one of its alternatives."""
    row: int
    col: int
    original_digit: int
    new_digit: int
    original_confidence: float
    alternative_confidence: float


@dataclass
class ResolutionResult:
    success: bool
    cells: List[CellInfo]
    grid: List[List[int]]
    corrections_made: List[CorrectionCandidate]
    paths_explored: int
    validation_result: ValidationResult
    score: float = 0.0


class ConflictResolver:
    """Beam search over the cells' alternatives for the cheapest set of corrections that satisfies the sudoku rules."""

    def __init__(self, beam_width: int = 5, max_corrections: int = 3, min_alternative_confidence: float = 0.1):
        self.beam_width = beam_width
        self.max_corrections = max_corrections
        self.min_alternative_confidence = min_alternative_confidence

    def resolve(self, cells: List[CellInfo]) -> ResolutionResult:
        out = device_resolve(cells, self.beam_width, self.max_corrections, self.min_alternative_confidence)
        made = [CorrectionCandidate(row=int(x) // 9, col=int(x) % 9, original_digit=int(old), new_digit=int(new),
                                    original_confidence=float(c0), alternative_confidence=float(c1))
                for (x, old, new), (c0, c1) in zip(out["corr_cells"][:int(out["n_corrections"])], out["corr_conf"])]
        if made:
            index, prob = out["index"], out["prob"]
            new_cells = [CellInfo(row=c.row, col=c.col, digit=int(index[9 * c.row + c.col, 0]), confidence=float(prob[9 * c.row + c.col, 0]),
                                  alternatives=[(int(d), float(p)) for d, p in zip(index[9 * c.row + c.col, 1:], prob[9 * c.row + c.col, 1:]) if d != _NONE])
                         for c in cells]
        else:
            new_cells = cells          # valid as it is, or nothing to try: the reference hands the caller's list back too
        digits = out["digits"]
        return ResolutionResult(success=bool(out["success"]), cells=new_cells, grid=[[int(digits[9 * r + c]) for c in range(9)] for r in range(9)],
                                corrections_made=made, paths_explored=int(out["paths_explored"]),
                                validation_result=validation_from(digits, out["num_conflicts_after"], out["conflict_count"]),
                                score=float(out["score"]))


def resolve_conflicts(cells: List[CellInfo], beam_width: int = 5, max_corrections: int = 3) -> ResolutionResult:
    """pipeline/run_v2.py:355-359."""
    return ConflictResolver(beam_width=beam_width, max_corrections=max_corrections).resolve(cells)
