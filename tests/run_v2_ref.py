"""The stages of run_v2 (pipeline/run_v2.py:276-407) chained on the CPU.  TEST INFRASTRUCTURE ONLY.

`chain` restates the call order and the hand-offs of run_v2's run_pipeline and nothing else: every stage is one of the independent
restatements the suite already holds its kernels against, and no arithmetic is added here beyond a float64 softmax with a stable
descending order.  It does not import the library (overlay_ref.font_atlas reads the library's glyph table, as it does for
tests/test_gpu_overlay.py; pass `atlas` to avoid even that).

    preprocess_v2_ref.preprocess_multi_strategy(image)          :279     binary; its `gray` is the gray of the image itself (:276)
    grid_v2_ref.detect_grid(binary, gray)                       :287     corners, or the chain ends (:289-292)
    quality_ref.ref_assess(image, binary, corners)              :301     on the SAME binary and corners
    warp_ref.cells(image, Minv(corners))                        :314-318 of the image, not of anything preprocessed
    cnn_oracle.glue -> model_v3_ref.forward64 / forward         :161-167
    softmax(logits), no temperature; top-3, best first          :168-180
    resolve_ref.resolve + the acceptance rule                   :347-371
    constraint_ref.propagate(resolved digits, THEIR confidences):374-375
    solve_ref.solve(propagated grid) iff the propagation is valid :384-396
    overlay_ref.render(image, M(corners), solution minus the solver's input) iff solved

grid_v2_ref's last method draws from numpy's global generator; `chain` seeds it with 0 first, and a caller comparing against the library
does the same before its own call."""
import numpy as np

import cnn_oracle
import constraint_ref
import grid_v2_ref
import model_v3_ref
import overlay_ref
import preprocess_v2_ref
import quality_ref
import resolve_ref
import solve_ref
import sv_oracle
import warp_ref

GRID = 450


def minv_of(corners):
    """Destination -> source map of the 450 x 450 warp at `corners` (float32 [4,2], any order): the C oracle's."""
    return sv_oracle.corners_to_minv(np.asarray(corners, np.float32), GRID)


def m_of(corners):
    """Frame -> grid map at `corners`: cv2.getPerspectiveTransform of the ordered corners onto the square, the C oracle's."""
    s = np.float32(GRID - 1)
    return sv_oracle.get_perspective_transform(sv_oracle.order_points(np.asarray(corners, np.float32)), np.array([0, 0, s, 0, s, s, 0, s], np.float32))


def softmax64(logits):
    z = np.asarray(logits, np.float64)
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def top3(logits, k=3):
    """float64 softmax, stable descending order (equal probabilities: lowest class first) -> (index u8 [n,k], prob f64 [n,k], p [n,10])."""
    p = softmax64(logits)
    order = np.argsort(-p, axis=-1, kind="stable")[..., :k]
    return order.astype(np.uint8), np.take_along_axis(p, order, -1), p


def validate_and_resolve(index, prob):
    """run_v2.py:347-371 on one frame's top-k (index u8 [81,k], prob f32 [81,k]) -> dict: validation (of the cells run_v2 goes on with),
    corrections [(row, col, old, new, old confidence, new confidence)], digits u8 [81], conf f32 [81], paths_explored."""
    index, prob = np.asarray(index, np.uint8), np.asarray(prob, np.float32)
    r = {k: v[0] for k, v in resolve_ref.resolve(index[None], prob[None]).items()}
    digits, conf, corrections = index[:, 0].copy(), prob[:, 0].copy(), []
    if r["num_conflicts_before"] and (r["success"] or r["num_conflicts_after"] < r["num_conflicts_before"]):        # :365
        digits, conf = r["digits"], r["conf"]
        corrections = [(int(x) // 9, int(x) % 9, int(old), int(new), float(c0), float(c1))
                       for (x, old, new), (c0, c1) in zip(r["corr_cells"][:int(r["n_corrections"])], r["corr_conf"])]
    n, count, _ = resolve_ref.validate([int(v) for v in digits])
    return {"validation": {"is_valid": n == 0, "num_conflicts": n, "cells_in_conflict": [(x // 9, x % 9) for x in range(81) if count[x]]},
            "corrections": corrections, "digits": digits, "conf": conf, "paths_explored": int(r["paths_explored"])}


def propagation_of(digits, conf):
    """constraint_ref.propagate of one frame -> (the `propagation` dict of the library's result, grid u8 [81], every field)."""
    p = {k: v[0] for k, v in constraint_ref.propagate(np.asarray(digits, np.uint8)[None], np.asarray(conf, np.float32)[None]).items()}
    bad = int(p["contradiction_cell"])
    shown = {"is_valid": bool(p["is_valid"]), "iterations": int(p["iterations"]),
             "contradiction_cell": None if bad == constraint_ref.NONE else (bad // 9, bad % 9),
             "cells_resolved": [(int(x) // 9, int(x) % 9, int(v)) for x, v in p["resolved"][:int(p["n_resolved"])]]}
    return shown, p["grid"], p


def solve_of(grid, valid=True):
    """run_v2.py:384-407: the solver on `grid` iff the propagation was valid -> (result, solution u8 [81], nodes)."""
    grid = np.asarray(grid, np.uint8).reshape(81)
    if not valid:
        return solve_ref.SKIPPED, grid.copy(), 0
    code, solution, nodes = solve_ref.solve(grid)[:3]
    return int(code), np.asarray(solution).astype(np.uint8), int(nodes)


def overlay_of(image, corners, given, solution, solved, atlas=None):
    """The image with the cells of `solution` that `given` leaves empty drawn at `corners` when solved, else an unchanged copy."""
    if not solved:
        return np.array(image, np.uint8)
    given, solution = np.asarray(given, np.uint8).reshape(81), np.asarray(solution, np.uint8).reshape(81)
    digits = np.where(given != 0, 0, solution).astype(np.uint8)
    return overlay_ref.render(image, m_of(corners), digits, None, None, overlay_ref.font_atlas() if atlas is None else atlas)


def front(image, glue=1):
    """run_v2.py:276-318: everything before the model -> dict(preprocess, binary, gray, detection, corners, quality, cells, x); the last
    four are None where no grid is found."""
    image = np.ascontiguousarray(image, np.uint8)
    pre = preprocess_v2_ref.preprocess_multi_strategy(image)
    np.random.seed(0)
    det = grid_v2_ref.detect_grid(pre["binary"], pre["gray"])
    out = {"image": image, "preprocess": pre, "binary": pre["binary"], "gray": pre["gray"], "detection": det, "corners": det["corners"],
           "quality": None, "cells": None, "x": None}
    if det["corners"] is None:
        return out
    out["quality"] = quality_ref.ref_assess(image, pre["binary"], det["corners"])
    out["cells"] = warp_ref.cells(image, minv_of(det["corners"]))
    out["x"] = cnn_oracle.glue(out["cells"], glue)
    return out


def back(f, sd_v3, atlas=None):
    """run_v2.py:326-407 on front()'s result: adds logits64, logits32, index, prob (f64), prob32, digits, resolved (validate_and_resolve's
    dict), propagation, propagated, propagation_fields, solve_result, solution, solve_nodes, overlay."""
    out = dict(f)
    if f["corners"] is None:
        return out
    out["logits64"] = model_v3_ref.forward64(sd_v3, f["x"]).numpy()
    out["logits32"] = model_v3_ref.forward(sd_v3, f["x"]).numpy().astype(np.float64)
    out["index"], out["prob"], out["p"] = top3(out["logits64"])
    out["prob32"] = out["prob"].astype(np.float32)
    out["digits"] = out["index"][:, 0].copy()
    out["resolved"] = r = validate_and_resolve(out["index"], out["prob32"])
    out["propagation"], out["propagated"], out["propagation_fields"] = propagation_of(r["digits"], r["conf"])
    out["solve_result"], out["solution"], out["solve_nodes"] = solve_of(out["propagated"], out["propagation"]["is_valid"])
    out["overlay"] = overlay_of(f["image"], f["corners"], out["propagated"], out["solution"], out["solve_result"] == solve_ref.SOLVED, atlas)
    return out


def chain(image, sd_v3, glue=1, atlas=None):
    """image u8 [H,W,3] BGR, sd_v3 a DigitCNNv3 state dict -> every intermediate of run_v2's pipeline (front + back)."""
    return back(front(image, glue), sd_v3, atlas)
