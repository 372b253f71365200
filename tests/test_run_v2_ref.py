"""CPU: the chained reference of run_v2 (tests/run_v2_ref.py) and the scenarios built on it (tests/run_v2_cases.py), before anything
runs on a GPU: 1 the chain hands each stage what run_v2 hands it, 2 each scenario reaches the branch it is built for, 3 the scenarios
tell a right hand-off from the wrong one a pipeline could plausibly make (so that tests/test_gpu_run_v2_chain.py can), 4 the fitted
head: fit and margins."""
import ast
import os

import numpy as np
import pytest

import cnn_oracle
import constraint_ref
import model_v3_ref
import preprocess_v2_ref
import resolve_ref
import run_v2_cases as cases
import run_v2_ref as R
import solve_ref
import sv_oracle

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- 1: the chain ---------------------------------------------------------------------------------------------------------------------
def test_chain_does_not_import_the_library():
    tree = ast.parse(open(os.path.join(HERE, "run_v2_ref.py")).read())
    names = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    names += [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert names and not [n for n in names if n.split(".")[0] in ("sudoku_vision_amd", "torch")], names


def test_chain_returns_every_intermediate():
    ch = cases.scenario("solved")["chain"]
    assert {"binary", "gray", "corners", "cells", "logits64", "logits32", "index", "prob", "resolved", "propagation", "propagated",
            "solve_result", "solution", "overlay", "quality", "preprocess", "detection"} <= set(ch)
    image = cases.scenario("solved")["image"]
    assert ch["binary"].shape == ch["gray"].shape == image.shape[:2] and (ch["gray"] == sv_oracle.gray(image)).all()       # seam 1: the ORIGINAL's gray
    assert ch["cells"].shape == (81, 28, 28) and ch["logits64"].shape == (81, 10) and ch["index"].shape == (81, 3)
    assert (ch["prob"][:, :-1] > ch["prob"][:, 1:]).all() and np.abs(ch["p"].sum(1) - 1).max() < 1e-12
    assert ch["overlay"].shape == image.shape and ch["overlay"].dtype == np.uint8


def test_top3_is_a_stable_descending_order():
    z = np.array([[0, 1, 1, 0, 3, 1, 0, 0, 0, 0], [2] * 10], np.float64)
    idx, prob, p = R.top3(z)
    assert idx.tolist() == [[4, 1, 2], [0, 1, 2]] and np.allclose(prob[1], 0.1) and prob[0, 1] == prob[0, 2]


def test_acceptance_rule_of_the_chain():
    """A repair that neither succeeds nor leaves fewer conflicts is dropped (:365): `invalid` is such a frame; `solved` is repaired."""
    inv, sol = cases.scenario("invalid")["chain"], cases.scenario("solved")["chain"]
    assert inv["resolved"]["corrections"] == [] and (inv["resolved"]["digits"] == inv["digits"]).all() and not inv["resolved"]["validation"]["is_valid"]
    assert inv["resolved"]["validation"]["num_conflicts"] == resolve_ref.validate([int(v) for v in inv["digits"]])[0] >= 1
    assert len(sol["resolved"]["corrections"]) == 2 and sol["resolved"]["validation"] == {"is_valid": True, "num_conflicts": 0, "cells_in_conflict": []}
    for r, c, old, new, c_old, c_new in sol["resolved"]["corrections"]:
        x = 9 * r + c
        assert (old, new) == (int(sol["index"][x, 0]), int(sol["index"][x, 1])) and (c_old, c_new) == (float(sol["prob32"][x, 0]), float(sol["prob32"][x, 1]))
        assert sol["resolved"]["conf"][x] == sol["prob32"][x, 1]                # seam 5: the repaired cell carries the alternative's confidence


# ---- 2: the branch each scenario reaches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("solved", "solved_t2.5"))
def test_solved_reaches_the_solver_and_the_overlay(name):
    s = cases.scenario(name)
    ch = s["chain"]
    puzzle, solution = cases.golden_puzzle()
    assert (ch["digits"] == s["read"]).all() and (s["read"] != puzzle).sum() == 2
    assert resolve_ref.validate([int(v) for v in ch["digits"]])[0] >= 2                 # two units conflict at least
    assert len(ch["resolved"]["corrections"]) >= 1 and (ch["resolved"]["digits"] == puzzle).all() and ch["resolved"]["validation"]["is_valid"]
    assert ch["propagation"]["is_valid"] and len(ch["propagation"]["cells_resolved"]) >= 3
    assert ch["solve_result"] == solve_ref.SOLVED and (ch["solution"] == solution).all() and ch["solve_nodes"] > 1
    assert (ch["overlay"] != s["image"]).any()
    # the runner-up was eligible only because the misread cells are read unsurely
    for x in s["unsure"]:
        assert ch["prob"][x, 1] >= 0.1 > cases.scenario("unsolvable")["chain"]["prob"][:, 1].max()


def test_invalid_ends_before_the_solver():
    s = cases.scenario("invalid")
    ch = s["chain"]
    puzzle, _ = cases.golden_puzzle()
    (a,) = np.flatnonzero(s["read"] != puzzle)
    twin = [x for x in range(9 * (a // 9), 9 * (a // 9) + 9) if x != a and s["read"][x] == s["read"][a]]
    assert len(twin) == 1                                                              # the same digit twice in a row
    for x in (a, twin[0]):
        assert int(puzzle[a]) not in ch["index"][x].tolist()                           # the misread cell's truth is in neither cell's three
        assert ch["prob"][x, 1] < 0.1                                                  # and no alternative is eligible
    assert (ch["digits"] == s["read"]).all() and ch["resolved"]["corrections"] == []
    assert not ch["propagation"]["is_valid"] and ch["propagation"]["contradiction_cell"] is not None
    assert (ch["solve_result"], ch["solve_nodes"]) == (solve_ref.SKIPPED, 0) and (ch["solution"] == ch["propagated"]).all()
    assert (ch["overlay"] == s["image"]).all()


def test_unsolvable_is_consistent_and_has_no_solution():
    s = cases.scenario("unsolvable")
    ch = s["chain"]
    assert (ch["digits"] == s["read"]).all() and ch["resolved"]["validation"]["is_valid"] and ch["resolved"]["corrections"] == []
    assert ch["propagation"]["is_valid"] and len(ch["propagation"]["cells_resolved"]) >= 3
    assert ch["solve_result"] == solve_ref.NOSOLUTION and (ch["solution"] == ch["propagated"]).all()
    assert (ch["overlay"] == s["image"]).all()


def test_not_found_ends_at_the_detection():
    ch = cases.scenario("not_found")["chain"]
    assert ch["corners"] is None and ch["detection"]["method"] == "none" and ch["cells"] is None and "logits64" not in ch


def test_temperature_changes_nothing_the_chain_computes():
    a, b = cases.scenario("solved")["chain"], cases.scenario("solved_t2.5")["chain"]
    assert float(cases.scenario("solved_t2.5")["sd"]["temperature"]) == 2.5
    for key in ("logits64", "index", "prob", "propagated", "solution", "overlay"):
        assert np.array_equal(a[key], b[key]), key
    assert a["resolved"]["corrections"] == b["resolved"]["corrections"] and a["propagation"] == b["propagation"]


# ---- 3: the wrong hand-offs are visible on these frames -----------------------------------------------------------------------------------
def test_the_scenarios_tell_the_seams_apart():
    s = cases.scenario("solved")
    ch, image = s["chain"], s["image"]
    # seams 1 and 2: the v1 binary is another image, and so is the gray of the enhanced frame
    assert (sv_oracle.preprocess_for_grid_detection(image) != ch["binary"]).any()
    assert (ch["preprocess"]["enhanced"] != ch["gray"]).any()
    # seam 4: the temperature-scaled confidence is on the other side of the propagation's `> 0.9` in many cells
    z = ch["logits64"] / 2.5
    tempered = (np.exp(z - z.max(1, keepdims=True)) / np.exp(z - z.max(1, keepdims=True)).sum(1, keepdims=True)).max(1)
    fixed = ch["propagation_fields"]["is_fixed"]
    other = constraint_ref.propagate_one(ch["resolved"]["digits"], tempered.astype(np.float32))["is_fixed"]
    assert fixed.sum() >= 20 and other.sum() == 0
    # seam 5: propagating the unresolved digits ends elsewhere
    raw = R.propagation_of(ch["digits"], ch["prob32"][:, 0])
    assert raw[0] != ch["propagation"] and (raw[1] != ch["propagated"]).any()
    # seam 6: the solver on the resolved grid finds the same solution, and the overlay then draws the propagated cells too
    code, solution, _ = R.solve_of(ch["resolved"]["digits"])
    assert code == solve_ref.SOLVED and (solution == ch["solution"]).all()
    assert (R.overlay_of(image, ch["corners"], ch["resolved"]["digits"], solution, True) != ch["overlay"]).any()
    # seam 7: with the givens taken from the raw digits the cells the propagation filled are drawn too
    assert (R.overlay_of(image, ch["corners"], ch["digits"], ch["solution"], True) != ch["overlay"]).any()
    # seam 6, second half: a solver run on the invalid frame's grid would answer, not skip
    inv = cases.scenario("invalid")["chain"]
    assert R.solve_of(inv["propagated"])[0] != solve_ref.SKIPPED


# ---- 4: the fitted head -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.SYNTHETIC)
def test_fit_and_margins(name):
    s = cases.scenario(name)
    ch = s["chain"]
    fit = float(np.abs(ch["logits64"] - s["target"]).max())
    noise, tol, gap = cases.margins(ch["logits64"], ch["logits32"])
    print(f"FIT {name}: max|forward64 - target| {fit:.3e}; noise {noise:.3e} tol {tol:.3e} smallest gap {gap:.4f} = {gap / tol:.0f} tol")
    assert fit <= cases.FIT
    assert gap > cases.MARGIN * tol
    assert tol == cnn_oracle.tolerance(ch["logits64"], noise, model_v3_ref.C_V3)
    # the rest of the state dict is the random one, and the model really is the restated DigitCNNv3 on the chain's own cells
    base = model_v3_ref.random_state_dict_v3(2024, use_se=True)
    assert all((s["sd"][k] == base[k]).all() for k in base if not k.startswith("fc.") and k != "temperature")
    assert (ch["x"] == cnn_oracle.glue(ch["cells"], 1)).all()
    assert sorted(set(np.round(s["target"], 9).ravel().tolist())) in ([0.0, 3.0, 5.0, 8.0], [0.0, 3.0, 5.0, 6.0, 8.0])


def test_preprocess_and_detection_are_the_suites_own_restatements():
    s = cases.scenario("unsolvable")
    want = preprocess_v2_ref.preprocess_multi_strategy(s["image"])
    assert (want["binary"] == s["chain"]["binary"]).all() and want["method_used"] == s["chain"]["preprocess"]["method_used"]
    assert s["chain"]["detection"]["method"] == "contour" and s["chain"]["corners"].dtype == np.float32
