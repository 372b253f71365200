"""The frames and models tests/test_run_v2_ref.py (CPU) and tests/test_gpu_run_v2_chain.py (GPU) send through every stage of run_v2 at
once.  TEST INFRASTRUCTURE ONLY.

A random DigitCNNv3 reads noise and trained weights are not needed: for a given frame only the model's last layer is FITTED, on the CPU
in float64, so that the real CNN on the real warped cells reads a chosen grid with chosen alternatives:
    features   model_v3_ref.forward64(random_state_dict_v3(2024, use_se=True), glue(cells)) of the 81 cells the chained reference warps
               at its own corners
    target     per cell: top class TOP = +8, a chosen runner-up SECOND = +5, a chosen third THIRD = +3, the rest 0
    fc         numpy.linalg.lstsq([features, 1], target): 81 equations, 129 unknowns per class, the minimum-norm solution, kept as
               float64 tensors in the state dict (model_v3_ref evaluates them as they are; the library rounds them to float32 when it
               packs them, which is part of the error its tolerance covers)
A cell that is to be MISREAD with the truth as its runner-up gets TOP_UNSURE = +6 instead of +8: conflict repair only tries an
alternative of probability >= 0.1 (resolve_ref.candidates), and softmax gives the runner-up 0.047 under +8 / +5 / +3 but 0.26 under
+6 / +5 / +3.  Every other cell's alternatives stay below 0.1, so the repair can only take what the design offers.

What tests/test_run_v2_ref.py asserts of every fitted scenario before anything runs on a GPU:
    fit      max|forward64 logits - target| <= FIT = 1e-6
    margin   with noise = max|forward (f32) - forward64| and tol = cnn_oracle.tolerance(logits64, noise, model_v3_ref.C_V3), the rule
             tests/test_gpu_model_v3.py holds the GPU's logits to, every cell's gaps between ranks 1-2, 2-3 and 3-4 exceed 4 * tol:
             the GPU may move either side of a gap by tol, which leaves a factor of two on each side -- the discrete outputs of the
             GPU chain must then EQUAL the reference's.
"""
import functools
import os

import numpy as np
import torch

import cnn_oracle
import constraint_ref
import model_v3_ref
import resolve_ref
import run_v2_ref
import solve_ref

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 270, 480
TOP, TOP_UNSURE, SECOND, THIRD = 8.0, 6.0, 5.0, 3.0
FIT = 1e-6
MARGIN = 4.0
SEED = {"solved": 11, "invalid": 4, "unsolvable": 7}        # synth_frames seeds; a frame that fails the margin is replaced, not excused
GOLDEN_PUZZLE = 37          # of tests/golden/solver_golden.npz: 28 givens, propagation fills 10 cells, the solver then needs 10 nodes
SPARSE_UNSOLVABLE = 91      # of solve_ref.sparse_set(): consistent givens, propagation fills 10 cells and stays valid, no solution
SYNTHETIC = ("solved", "solved_t2.5", "invalid", "unsolvable")


def frame(seed):
    from sudoku_vision_amd.synth import synth_frames
    return synth_frames(1, H, W, seed=seed, device="cpu", noise="int")[0][0].numpy()


def flat_frame():
    return np.full((H, W, 3), 128, np.uint8)


def golden_puzzle():
    g = np.load(os.path.join(HERE, "golden", "solver_golden.npz"))
    assert g["codes"][GOLDEN_PUZZLE] == 1
    return g["puzzles"][GOLDEN_PUZZLE].reshape(81).astype(np.uint8), g["solutions"][GOLDEN_PUZZLE].reshape(81).astype(np.uint8)


def _conflicting_peer_digit(grid, x, avoid=()):
    """A digit some given peer of x shows (reading it at x makes a unit conflict), lowest first, not in `avoid`."""
    shown = sorted({int(grid[y]) for y in constraint_ref.PEERS[x] if grid[y]} - {int(grid[x])} - set(avoid))
    return shown[0]


def design(name):
    """-> (read u8 [81]: what the model is to read, second {cell: runner-up}, third {cell: third}, unsure: cells that get TOP_UNSURE,
    truth u8 [81]: the grid the stages after the repair should go on with)."""
    puzzle, _ = golden_puzzle()
    if name in ("solved", "solved_t2.5"):
        # two givens in different rows, columns and boxes, each read as a digit one of its peers shows: two units conflict at least.
        # The truth is the runner-up of both, so the repair needs two corrections and finds them
        givens = [x for x in range(81) if puzzle[x]]
        a = givens[2]
        b = next(x for x in givens if x // 9 != a // 9 and x % 9 != a % 9 and (x // 27, x % 9 // 3) != (a // 27, a % 9 // 3))
        read, second = puzzle.copy(), {}
        for x in (a, b):
            read[x] = _conflicting_peer_digit(puzzle, x)
            second[x] = int(puzzle[x])
        return read, second, {}, (a, b), puzzle
    if name == "invalid":
        # one given read as the digit another given of its row shows; the truth is in neither cell's alternatives, and at +8 / +5 / +3
        # no alternative reaches 0.1 anyway: nothing to try.  The pair is the first whose propagation ends in a contradiction
        for a in range(81):
            for b in range(9 * (a // 9), 9 * (a // 9) + 9):
                if a == b or not puzzle[a] or not puzzle[b] or puzzle[a] == puzzle[b]:
                    continue
                read = puzzle.copy()
                read[a] = puzzle[b]
                p = constraint_ref.propagate_one(read)
                if not p["is_valid"] and p["contradiction_cell"] != constraint_ref.NONE:
                    others = [d for d in range(1, 10) if d not in (puzzle[a], puzzle[b])]
                    return read, {a: others[0], b: others[1]}, {a: others[2], b: others[3]}, (), read
        raise AssertionError("no contradictory pair")
    if name == "unsolvable":
        grid = solve_ref.sparse_set()[SPARSE_UNSOLVABLE].copy()
        return grid, {}, {}, (), grid
    raise KeyError(name)


def target_logits(read, second, third, unsure):
    t = np.zeros((81, 10))
    for x in range(81):
        top = int(read[x])
        s = second.get(x, (top + 4) % 10)
        th = third.get(x, next(d for d in ((top + 7) % 10, (top + 8) % 10, (top + 9) % 10) if d not in (top, s)))
        assert len({top, s, th}) == 3
        t[x, top], t[x, s], t[x, th] = (TOP_UNSURE if x in unsure else TOP), SECOND, THIRD
    return t


def fitted_state_dict(x, target, temperature=1.0):
    """The DigitCNNv3 state dict whose fc layer maps the features of the cells x [81,1,28,28] onto `target` [81,10]."""
    sd = {k: v.clone() for k, v in model_v3_ref.random_state_dict_v3(2024, use_se=True).items()}
    _, feats = model_v3_ref.forward64(sd, x, return_features=True)
    A = np.concatenate([feats.numpy(), np.ones((len(x), 1))], 1)
    sol = np.linalg.lstsq(A, target, rcond=None)[0]
    sd["fc.weight"] = torch.from_numpy(np.ascontiguousarray(sol[:128].T))
    sd["fc.bias"] = torch.from_numpy(np.ascontiguousarray(sol[128]))
    sd["temperature"][:] = temperature
    return sd


def margins(logits64, logits32):
    """-> (noise, tol, the smallest gap between ranks 1-2, 2-3, 3-4 over the cells)."""
    noise = float(np.abs(logits32 - logits64).max())
    tol = cnn_oracle.tolerance(logits64, noise, model_v3_ref.C_V3)
    ranked = -np.sort(-logits64, 1)
    return noise, tol, float((ranked[:, :3] - ranked[:, 1:4]).min())


@functools.lru_cache(maxsize=None)
def _front(seed):
    return run_v2_ref.front(frame(seed))


@functools.lru_cache(maxsize=None)
def scenario(name):
    """-> dict(name, image, sd, target, read, truth, unsure, chain: run_v2_ref.chain's result); computed once, never changed."""
    if name == "not_found":
        image = flat_frame()
        sd = model_v3_ref.random_state_dict_v3(2024, use_se=True)
        return {"name": name, "image": image, "sd": sd, "chain": run_v2_ref.chain(image, sd)}
    f = _front(SEED["solved" if name == "solved_t2.5" else name])
    assert f["corners"] is not None, name
    read, second, third, unsure, truth = design(name)
    target = target_logits(read, second, third, unsure)
    sd = fitted_state_dict(f["x"], target, 2.5 if name == "solved_t2.5" else 1.0)
    chain = run_v2_ref.back(f, sd)
    for k, v in chain.items():
        if isinstance(v, np.ndarray) and k != "x":          # (torch wraps x without copying and wants it writable)
            v.setflags(write=False)
    return {"name": name, "image": f["image"], "sd": sd, "target": target, "read": read, "truth": truth, "unsure": unsure, "chain": chain}


def photo():
    """tests/golden/sample_1.jpg, every fourth pixel of the C oracle's decode (912 x 684), and the weights tests/golden/model_v3_se.npz
    was recorded with -> (image, state dict)."""
    import sv_oracle
    with open(os.path.join(HERE, "golden", "sample_1.jpg"), "rb") as f:
        image = np.ascontiguousarray(sv_oracle.imdecode(f.read())[::4, ::4])
    g = np.load(os.path.join(HERE, "golden", "model_v3_se.npz"))
    return image, model_v3_ref.random_state_dict_v3(int(g["w_seed"]), use_se=True)
