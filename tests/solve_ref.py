"""solver/src/sudoku.c restated in plain Python, function by function, with the two things K14 (csrc/k14_solve.hip) and
sv_solve_sudoku_batch_host add to it: a count of the search nodes and a budget for them.  Written from the C source: validate_grid
(sudoku.c:413-467), init_candidates (:226-247), eliminate_from_peers (:251-283), propagate (:287-401), solve_with_candidates (:6-59),
solve_sudoku (:72-81).  A node is one entry into solve_with_candidates; the root is node 1; a node that would be entered with
max_nodes already entered ends the puzzle with BUDGET (max_nodes == 0: no budget).

Also the puzzle sets the solver tests share: the goldens, the crafted cases, the seeded sparse set, and the hard set whose searches go
deep and leave branches, with its one budgeted run (capped) and the budgets derived from it (edge_cases, edge_budgets)."""
import functools
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOLVED, NOSOLUTION, INVALID, BUDGET, SKIPPED = 1, 0, -1, 2, 3
BUDGETS = (0, 1, 8, 48, 4096)


class _Budget(Exception):
    pass


def _eliminate_from_peers(cands, row, col, num):
    bit = ~(1 << num)
    for c in range(9):
        if c != col:
            cands[row][c] &= bit
    for r in range(9):
        if r != row:
            cands[r][col] &= bit
    br, bc = row // 3 * 3, col // 3 * 3
    for r in range(br, br + 3):
        for c in range(bc, bc + 3):
            if r != row or c != col:
                cands[r][c] &= bit


def _validate_grid(grid):
    for i in range(9):
        for j in range(9):
            if grid[i][j] < 0 or grid[i][j] > 9:
                return False
    units = [[(r, c) for c in range(9)] for r in range(9)] + [[(r, c) for r in range(9)] for c in range(9)] + \
            [[(r, c) for r in range(br, br + 3) for c in range(bc, bc + 3)] for br in (0, 3, 6) for bc in (0, 3, 6)]
    for unit in units:
        seen = 0
        for r, c in unit:
            val = grid[r][c]
            if val != 0:
                if seen & (1 << val):
                    return False
                seen |= 1 << val
    return True


def _init_candidates(grid):
    cands = [[0 if grid[i][j] != 0 else 0x3FE for j in range(9)] for i in range(9)]
    for i in range(9):
        for j in range(9):
            if grid[i][j] != 0:
                _eliminate_from_peers(cands, i, j, grid[i][j])
    return cands


def _set(grid, cands, r, c, num):
    grid[r][c] = num
    cands[r][c] = 0
    _eliminate_from_peers(cands, r, c, num)


def _hidden(grid, cands, cells, num):
    """One (unit, digit) step of the three hidden-single loops -> -1 contradiction, 1 placed, 0 nothing."""
    count, last = 0, None
    for r, c in cells:
        if grid[r][c] == num:
            count = -1
            break
        if grid[r][c] == 0 and cands[r][c] & (1 << num):
            count += 1
            last = (r, c)
    if count == 0:
        return -1
    if count == 1 and last is not None:
        _set(grid, cands, last[0], last[1], num)
        return 1
    return 0


_ROWS = [[(r, c) for c in range(9)] for r in range(9)]
_COLS = [[(r, c) for r in range(9)] for c in range(9)]
_BOXES = [[(r, c) for r in range(br, br + 3) for c in range(bc, bc + 3)] for br in (0, 3, 6) for bc in (0, 3, 6)]


def _propagate(grid, cands, stats):
    progress = True
    while progress:
        progress = False
        stats["sweeps"] += 1
        for i in range(9):
            for j in range(9):
                if grid[i][j] == 0:
                    count = bin(cands[i][j]).count("1")
                    if count == 0:
                        return -1
                    if count == 1:
                        _set(grid, cands, i, j, cands[i][j].bit_length() - 1)
                        progress = True
        for units in (_ROWS, _COLS, _BOXES):
            for cells in units:
                for num in range(1, 10):
                    r = _hidden(grid, cands, cells, num)
                    if r < 0:
                        return -1
                    if r > 0:
                        progress = True
    return 0


def _left(stats):
    """A node returns False: one more level left since the last node was entered."""
    stats["left"] += 1
    stats["most_left"] = max(stats["most_left"], stats["left"])
    return False


def _solve_with_candidates(grid, cands, stats, depth):
    if stats["max_nodes"] and stats["nodes"] == stats["max_nodes"]:
        raise _Budget
    stats["nodes"] += 1
    stats["depth"] = max(stats["depth"], depth)
    if stats["left"]:
        stats["reentries"] += 1
        stats["left"] = 0
    if _propagate(grid, cands, stats) < 0:
        return _left(stats)
    if all(grid[i][j] != 0 for i in range(9) for j in range(9)):
        return True
    best, min_count = None, 10
    for i in range(9):
        for j in range(9):
            if grid[i][j] == 0:
                count = bin(cands[i][j]).count("1")
                if count < min_count:
                    min_count, best = count, (i, j)
    if best is None:
        return _left(stats)
    cell_cands = cands[best[0]][best[1]]
    for num in range(1, 10):
        if cell_cands & (1 << num):
            grid_copy = [row[:] for row in grid]
            cands_copy = [row[:] for row in cands]
            _set(grid_copy, cands_copy, best[0], best[1], num)
            if _solve_with_candidates(grid_copy, cands_copy, stats, depth + 1):
                for i in range(9):
                    grid[i][:] = grid_copy[i]
                return True
    return _left(stats)


def solve(grid, max_nodes=0):
    """grid: 81 or 9x9 integers -> (result, solution int64 [81], nodes, depth, sweeps, most_left, reentries): solution = grid unless
    result is SOLVED; depth is the deepest node's (the root's is 1).  A level is left when its node returns without a solution:
    most_left is the most levels left between two consecutive node entries, or between the last entry and the end of a search that
    found nothing (a contradiction in a node whose parent has a digit left to try is 1; K14 pops most_left - 1 levels of its stack,
    since a node whose propagation fails is never pushed); reentries counts the nodes entered after a level was left, whose state
    therefore comes from an older level than the one entered last."""
    g0 = [int(v) for v in np.asarray(grid).reshape(81)]
    grid = [g0[9 * r:9 * r + 9] for r in range(9)]
    if not _validate_grid(grid):
        return INVALID, np.array(g0), 0, 0, 0, 0, 0
    stats = {"nodes": 0, "max_nodes": int(max_nodes), "depth": 0, "sweeps": 0, "left": 0, "most_left": 0, "reentries": 0}
    try:
        ok = _solve_with_candidates(grid, _init_candidates(grid), stats, 1)
    except _Budget:
        return BUDGET, np.array(g0), stats["nodes"], stats["depth"], stats["sweeps"], stats["most_left"], stats["reentries"]
    return ((SOLVED if ok else NOSOLUTION), np.array(sum(grid, []) if ok else g0), stats["nodes"], stats["depth"], stats["sweeps"],
            stats["most_left"], stats["reentries"])


# ---- puzzle sets --------------------------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("make_solver_goldens", os.path.join(HERE, "golden", "make_solver_goldens.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


def goldens():
    """-> [(name, puzzles int32 [n,9,9], codes, solutions)] of the two files the reference library's answers are recorded in."""
    out = []
    for name in ("solver_golden.npz", "solver_golden_seed99.npz"):
        g = np.load(os.path.join(HERE, "golden", name))
        out.append((name, g["puzzles"], g["codes"], g["solutions"]))
    return out


@functools.lru_cache(maxsize=None)
def sparse_set():
    """512 puzzles of make_solver_goldens.py's generator (seed 2024) with 17..30 clues: the first 256 it makes of its plain kinds and the
    first 256 of the kind with one clue falsified, interleaved -> uint8 [512,81]."""
    P = _generator().puzzles(seed=2024, n=16000)
    clues = (P != 0).reshape(len(P), 81).sum(1)
    kind = np.arange(len(P)) % 8
    fits = (clues >= 17) & (clues <= 30)
    plain, wrong = np.flatnonzero(fits & (kind < 6))[:256], np.flatnonzero(fits & (kind == 7))[:256]
    assert len(plain) == 256 and len(wrong) == 256
    out = np.empty((512, 81), np.uint8)
    out[0::2] = P[plain].reshape(256, 81)
    out[1::2] = P[wrong].reshape(256, 81)
    return out


HARD_SEEDS = (("inkala", "8..........36......7..9.2...5...7.......457.....1...3...1....68..85...1..9....4.."),
              ("impossible", ".....5.8....6.1.43..........1.5........1.6...3.......553.....61........4........."),
              ("hard1", "4.....8.5.3..........7......2.....6.....8.4......1.......6.3.7.5..2.....1.4......"))
HARD_MORPHS = 24
HARD_CAP = 4096


def _morph(g, rng):
    """A symmetry of the grid (transpose, rows within bands, bands, the same for columns, a relabelling of the digits): as solvable
    as g, but another row-major, ascending-digit decision order, so another search tree."""
    G = g.reshape(9, 9).copy()
    if rng.integers(2):
        G = G.T.copy()

    def perm():
        return np.concatenate([3 * b + rng.permutation(3) for b in rng.permutation(3)])
    G = G[perm()][:, perm()]
    relabel = np.concatenate([[0], rng.permutation(9) + 1]).astype(np.uint8)
    return relabel[G].reshape(81)


@functools.lru_cache(maxsize=None)
def hard_set():
    """Puzzles whose search goes deep and leaves branches: the three seeds of HARD_SEEDS, then 24 morphs of each from one
    default_rng(11) consumed in that order -> uint8 [75,81].  Seed k is puzzle k; its morph m is puzzle 3 + 24 * k + m.  The
    `impossible` family has no solution, and most of its members do not show that within any budget the entries take."""
    seeds = [np.array([0 if ch == "." else int(ch) for ch in text], np.uint8) for _, text in HARD_SEEDS]
    assert all(s.shape == (81,) for s in seeds)
    rng = np.random.default_rng(11)
    morphs = [_morph(s, rng) for s in seeds for _ in range(HARD_MORPHS)]
    return np.stack(seeds + morphs).astype(np.uint8)


FULL = np.array([[(3 * (r % 3) + r // 3 + c) % 9 + 1 for c in range(9)] for r in range(9)], np.uint8)     # a valid filled grid


def crafted():
    """-> (names, grids uint8 [m,81]) of the hand-made cases (the backtracking one comes from the sparse set: see backtracking_case)."""
    cases = {}
    cases["empty"] = np.zeros((9, 9), np.uint8)
    cases["full"] = FULL.copy()
    g = FULL.copy()
    g[4, 4] = g[4, 5]
    cases["full_duplicate"] = g
    g = np.zeros((9, 9), np.uint8)
    g[2, 7] = 10
    cases["value_10"] = g
    # (0,0) and (0,1) are peers and both are left with 9 alone: row 0 shows 1..7, column 0 and column 1 each show an 8 further down
    g = np.zeros((9, 9), np.uint8)
    g[0, 2:9] = [1, 2, 3, 4, 5, 6, 7]
    g[3, 0] = 8
    g[6, 1] = 8
    cases["peers_same_sole_candidate"] = g
    # in row 0 the digits 1 and 2 both have (0,0) as their only place: columns 1..8 of the row are closed to both by a 1 and a 2 in
    # each of those columns or their boxes, and (0,0) keeps both as candidates
    g = np.zeros((9, 9), np.uint8)
    g[1, 3], g[2, 6] = 1, 1                    # boxes 1 and 2 of the top band closed to 1
    g[2, 3], g[1, 6] = 2, 2                    # and to 2
    g[3, 1], g[4, 2] = 1, 2                    # columns 1 and 2
    g[7, 1], g[6, 2] = 2, 1
    cases["two_digits_one_cell"] = g
    names = list(cases)
    return names, np.stack([cases[k].reshape(81) for k in names])


@functools.lru_cache(maxsize=None)
def unbounded(which):
    """The restatement without a budget on a whole set ('sparse', 'crafted', 'golden0', 'golden1') -> (result int8 [n], solution uint8
    [n,81], nodes int32 [n], depth int32 [n]); the puzzles as int64 [n,81] come from puzzles_of."""
    P = puzzles_of(which)
    rows = [solve(p) for p in P]
    return (np.array([r[0] for r in rows], np.int8), np.stack([np.clip(r[1], 0, 255) for r in rows]).astype(np.uint8),
            np.array([r[2] for r in rows], np.int32), np.array([r[3] for r in rows], np.int32))


def puzzles_of(which):
    if which == "sparse":
        return sparse_set().astype(np.int64)
    if which == "crafted":
        return crafted()[1].astype(np.int64)
    if which == "hard":
        return hard_set().astype(np.int64)
    return goldens()[int(which[-1])][1].reshape(-1, 81).astype(np.int64)


def as_bytes(P):
    """What a caller hands the byte entries: out-of-range entries clipped to 255 (still invalid)."""
    return np.clip(P, 0, 255).astype(np.uint8)


def expected(which, max_nodes):
    """The restatement's (result, solution, nodes) on a set under a budget.  A puzzle whose unbounded run enters no more nodes than the
    budget never consults it, so its unbounded answer stands; the others are run again with the budget."""
    res, sol, nodes, _ = (a.copy() for a in unbounded(which))
    if max_nodes:
        P = puzzles_of(which)
        for i in np.flatnonzero(nodes > max_nodes):
            r = solve(P[i], max_nodes)
            res[i], sol[i], nodes[i] = r[0], np.clip(r[1], 0, 255), r[2]
    return res, sol, nodes


@functools.lru_cache(maxsize=None)
def capped(which, cap):
    """One run of the restatement on a whole set under a budget of cap nodes, for the sets unbounded() cannot finish ('hard': some
    45 s at 4096) -> (result int8 [n], solution uint8 [n,81], nodes int32 [n], depth int32 [n], most_left int32 [n], reentries int32
    [n]).  Shared: leave the arrays as they are."""
    assert cap > 0
    rows = [solve(p, cap) for p in puzzles_of(which)]
    return (np.array([r[0] for r in rows], np.int8), np.stack([np.clip(r[1], 0, 255) for r in rows]).astype(np.uint8),
            *(np.array([r[k] for r in rows], np.int32) for k in (2, 3, 5, 6)))


def expected_capped(which, cap, b):
    """The restatement's (result, solution, nodes) on a set under a budget 1 <= b <= cap, from the capped run alone: the search is
    deterministic, so a run under b is the first b nodes of a run under cap (tests/test_solve_ref.py::test_budget_is_a_prefix).  A
    puzzle whose capped run ended by itself within b nodes keeps its answer; every other one spends the budget."""
    assert 1 <= b <= cap
    res, sol, nodes = (a.copy() for a in capped(which, cap)[:3])
    spent = (res == BUDGET) | ((res != INVALID) & (nodes > b))
    res[spent], nodes[spent] = BUDGET, b
    sol[spent] = as_bytes(puzzles_of(which))[spent]
    return res, sol, nodes


def edge_cases(res, nodes):
    """From a run of the hard set under HARD_CAP (the restatement's or the host's, which tests/test_solve_ref.py holds equal) ->
    [(name, puzzle, k)]: every puzzle refuted within the cap, the solved puzzles with the most and the fewest nodes and inkala itself,
    each with its node count k.  Budget k is the least that lets the puzzle end by itself, k - 1 the largest it spends."""
    refuted = np.flatnonzero(res == NOSOLUTION)
    solved = np.flatnonzero(res == SOLVED)
    assert len(refuted) >= 2 and len(solved) >= 2 and res[0] == SOLVED
    picks = [(f"refuted{j}", int(i)) for j, i in enumerate(refuted)]
    picks += [("most", int(solved[np.argmax(nodes[solved])])), ("fewest", int(solved[np.argmin(nodes[solved])])), ("inkala", 0)]
    return [(name, i, int(nodes[i])) for name, i in picks]


def edge_budgets(res, nodes):
    """-> the budgets the hard set is run under beside HARD_CAP, ascending: k and k - 1 of every edge case, and four fixed ones."""
    ks = {b for _, _, k in edge_cases(res, nodes) for b in (k, k - 1) if b >= 1}
    return tuple(sorted(ks | {48, 49, 256, 1024}))


@functools.lru_cache(maxsize=None)
def backtracking_case():
    """Index into the sparse set of the first solvable puzzle that has to leave a wrong branch: more nodes than its deepest level."""
    for i, p in enumerate(sparse_set()):
        res, _, nodes, depth = solve(p)[:4]
        if res == SOLVED and nodes > depth:
            return i
    raise AssertionError("the sparse set holds no puzzle that backtracks")
