"""Drop-in for the reference's pipeline/constraint_resolver.py: the names, fields, argument names and defaults that pipeline/run_v2.py:43
imports, with the propagation itself on the MI355X (sv_propagate_constraints, csrc/k10_propagate.hip): one launch per propagate(),
every field of the result equal to the reference's -- cells_resolved in the reference's order, each cell's candidates, and the
verdict on contradictory grids, where the reference's result depends on the order of a CPython set, which the kernel replays.

Confidences are rounded to float32 on the way in, because that is what the device holds (is_fixed is `float32 value > 0.9`); run_v2
only ever passes float32 softmax outputs, for which this changes nothing.  Cell.confidence is the caller's own value.
A resolver propagates once: a second propagate() raises, and get_candidates answers from the propagated state, so it raises before
propagate().  try_value, find_naked_singles, find_hidden_singles and _set_cell are not provided (run_v2 uses none of them).
max_iterations is 1..100 (the library refuses anything else).  There is no CPU fallback.
"""
import os
import sys
from dataclasses import dataclass, field
from typing import List, Optional, Set, Tuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bootstrap import package  # noqa: E402
sys.path.pop(0)
_rt = package().runtime

_NONE = 255                       # no contradiction cell (include/sudoku_vision_hip.h, sv_propagate_constraints)


@dataclass
class Cell:
    """Cell with candidates."""
    row: int
    col: int
    value: int                    # 0 if not set
    candidates: Set[int] = field(default_factory=lambda: set(range(1, 10)))
    confidence: float = 1.0
    is_fixed: bool = False

    def __hash__(self):
        return hash((self.row, self.col))


@dataclass
class PropagationResult:
    """Result of constraint propagation."""
    grid: List[List[int]]
    cells: List[Cell]
    cells_resolved: List[Tuple[int, int, int]]
    iterations: int
    is_valid: bool
    contradiction_cell: Optional[Tuple[int, int]] = None


class ConstraintResolver:
    """Naked and hidden singles until nothing moves."""

    def __init__(self, grid: List[List[int]], confidences: Optional[List[List[float]]] = None):
        self.original_grid = [row[:] for row in grid]
        g = np.array(grid, dtype=np.int64)
        if g.shape != (9, 9) or g.min() < 0 or g.max() > 9:
            raise ValueError("grid must be 9x9 with values 0..9")
        self._digits = g.astype(np.uint8).reshape(1, 81)
        self._confidences = [list(row) for row in confidences] if confidences else None
        self._conf = np.array(self._confidences, dtype=np.float32).reshape(1, 81) if confidences else None
        self._cells = None

    def propagate(self, max_iterations: int = 100) -> PropagationResult:
        if self._cells is not None:
            raise RuntimeError("ConstraintResolver (MI355X): a resolver propagates once; make a new one from the result's grid")
        ctx = _rt.default_context()
        conf = None if self._conf is None else torch.from_numpy(self._conf).to(ctx.device)
        out = {k: v[0].cpu().numpy() for k, v in ctx.propagate_constraints(torch.from_numpy(self._digits).to(ctx.device), conf, max_iterations).items()}
        grid, cand = out["grid"], out["candidates"]
        self._cells = [Cell(row=x // 9, col=x % 9, value=int(grid[x]), candidates={d for d in range(1, 10) if int(cand[x]) >> d & 1},
                            confidence=self._confidences[x // 9][x % 9] if self._confidences else 1.0, is_fixed=bool(out["is_fixed"][x]))
                       for x in range(81)]
        bad = int(out["contradiction_cell"])
        return PropagationResult(grid=[[int(grid[9 * r + c]) for c in range(9)] for r in range(9)], cells=list(self._cells),
                                 cells_resolved=[(int(x) // 9, int(x) % 9, int(v)) for x, v in out["resolved"][:int(out["n_resolved"])]],
                                 iterations=int(out["iterations"]), is_valid=bool(out["is_valid"]),
                                 contradiction_cell=None if bad == _NONE else (bad // 9, bad % 9))

    def get_candidates(self, row: int, col: int) -> Set[int]:
        if self._cells is None:
            raise RuntimeError("ConstraintResolver (MI355X): candidates exist on the device; call propagate() first")
        return self._cells[9 * row + col].candidates.copy()


def resolve_with_constraints(grid: List[List[int]], confidences: Optional[List[List[float]]] = None) -> PropagationResult:
    """pipeline/run_v2.py:375."""
    return ConstraintResolver(grid, confidences).propagate()
