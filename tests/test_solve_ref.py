"""CPU: the solver's batch entry on the host (sv_solve_sudoku_batch_host, csrc/host_solver.cpp) == the plain-Python restatement of
solver/src/sudoku.c (tests/solve_ref.py) in result, solution and node count, with and without a node budget; the restatement itself
== the reference library's recorded answers (tests/golden/solver_golden*.npz) and, where oracle/_ref is built, the library live."""
import ctypes as C
import os

import numpy as np
import pytest

import solve_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ("golden0", "golden1", "crafted", "sparse")


@pytest.fixture(scope="module")
def host():
    import sudoku_vision_amd as sva
    sva._native.lib()
    return sva.host


def test_restatement_reproduces_the_goldens():
    for k, (name, P, codes, sols) in enumerate(sr.goldens()):
        res, sol, nodes, _ = sr.unbounded(f"golden{k}")
        assert (res == codes).all(), name
        solved = codes == 1
        assert (sol[solved] == sols.reshape(-1, 81)[solved]).all(), name
        assert (sol[~solved] == sr.as_bytes(P.reshape(-1, 81))[~solved]).all(), name
        assert (nodes[codes == -1] == 0).all() and (nodes[codes != -1] >= 1).all()
        assert set(codes.tolist()) == {-1, 0, 1}


def test_crafted_cases_are_what_they_claim():
    names, grids = sr.crafted()
    res, sol, nodes, _ = sr.unbounded("crafted")
    got = {n: (int(r), int(k)) for n, r, k in zip(names, res, nodes)}
    assert got["empty"][0] == 1 and got["full"] == (1, 1) and got["full_duplicate"] == (-1, 0) and got["value_10"] == (-1, 0)
    # a contradiction inside the root's propagation: no branch is ever taken
    assert got["peers_same_sole_candidate"] == (0, 1) and got["two_digits_one_cell"] == (0, 1)
    assert (sol[names.index("full")] == grids[names.index("full")]).all()
    i = sr.backtracking_case()
    r = sr.solve(sr.sparse_set()[i])
    assert r[0] == 1 and r[2] > r[3]


def test_sparse_set_is_sparse_and_half_falsified():
    P = sr.sparse_set()
    clues = (P != 0).sum(1)
    assert P.shape == (512, 81) and clues.min() >= 17 and clues.max() <= 30
    res = sr.unbounded("sparse")[0]
    assert set(res.tolist()) == {-1, 0, 1} and (res[0::2] == 1).all()            # a puzzle with nothing falsified has a solution
    # where oracle/_ref is built: the reference library itself, live, on the same set (codes and solutions: it counts no nodes)
    ref = os.path.join(ROOT, "oracle", "_ref", "libsudoku_ref.so")
    if os.path.exists(ref):
        codes, grids = sr._generator().solve_all(C.CDLL(ref), P.reshape(-1, 9, 9).astype(np.int32))
        solved = codes == 1
        assert (codes == res).all() and (grids.reshape(-1, 81)[solved] == sr.unbounded("sparse")[1][solved]).all()


def test_default_budget_is_never_spent():
    """The condition behind Context.solve_sudoku's default of 4096 nodes: no frame of these sets comes near it; and each smaller budget
    the tests use is spent by some frame, so the budget path runs."""
    most = max(int(sr.unbounded(which)[2].max()) for which in SETS)
    print("nodes at most:", {which: int(sr.unbounded(which)[2].max()) for which in SETS})
    assert most <= 48 < 4096
    for budget in (1, 8):
        assert any((sr.expected(which, budget)[0] == sr.BUDGET).any() for which in SETS), budget
    for which in SETS:
        assert not (sr.expected(which, 48)[0] == sr.BUDGET).any() and not (sr.expected(which, 4096)[0] == sr.BUDGET).any()


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("max_nodes", sr.BUDGETS)
def test_host_batch_matches_the_restatement(host, which, max_nodes):
    P = sr.as_bytes(sr.puzzles_of(which))
    want = sr.expected(which, max_nodes)
    one = host.solve_sudoku_batch(P, max_nodes=max_nodes, threads=1)
    many = host.solve_sudoku_batch(P.reshape(-1, 9, 9), max_nodes=max_nodes, threads=16)
    for got in (one, many):
        assert got[0].dtype == np.int8 and got[1].dtype == np.uint8 and got[2].dtype == np.int32 and got[1].shape == (len(P), 9, 9)
        assert (got[0] == want[0]).all() and (got[1].reshape(-1, 81) == want[1]).all() and (got[2] == want[2]).all()
    spent = want[0] == sr.BUDGET
    assert (want[2][spent] == max_nodes).all() and (want[1][spent] == P[spent]).all()
    if max_nodes in (1, 8) and which != "crafted":
        assert spent.any()


# ---- the hard set: searches that go deep, leave branches several levels at once, refute after thousands of nodes or spend the budget -----
def test_hard_set_is_hard():
    """Conditions on the inputs, on the restatement alone: what the hard set has to be for the tests below (and those of
    tests/test_gpu_solve.py) to run the unwinding of the search at all."""
    P = sr.hard_set()
    assert P.shape == (75, 81) and P.dtype == np.uint8 and len({p.tobytes() for p in P}) == 75
    assert ((P != 0).sum(1)[3:].reshape(3, 24) == (P != 0).sum(1)[:3, None]).all()          # a morph keeps the number of clues
    res, sol, nodes, depth, left, reentries = sr.capped("hard", sr.HARD_CAP)
    print("puzzle: (result, nodes, depth, most levels left at once, entries after a return)")
    for i in range(75):
        name = sr.HARD_SEEDS[i][0] if i < 3 else f"{sr.HARD_SEEDS[(i - 3) // 24][0]}/{(i - 3) % 24}"
        print(f"  {i:2d} {name:14s} ({res[i]}, {nodes[i]}, {depth[i]}, {left[i]}, {reentries[i]})")
    print("most levels left at once:", int(left.max()), " entries after a return, most:", int(reentries.max()))
    assert set(res.tolist()) == {0, 1, 2}
    assert ((res == 0) & (nodes > 1000)).sum() >= 2
    assert ((res == 2) & (depth >= 16)).sum() >= 10
    assert ((res == 1) & (nodes >= 4 * depth)).sum() >= 20
    assert left.max() >= 2
    # the end of an exhaustive refutation leaves every level above its last node, which lies below the root; and from 3 on K14 pops
    # more than one level of its stack at once (a node whose propagation fails was never pushed)
    assert (left[res == 0] >= 2).all() and (left >= 3).sum() >= 10
    assert (reentries[nodes > 1000] > 500).all()                         # the long searches restore an older level all the time
    assert (nodes[res == 2] == sr.HARD_CAP).all() and (sol[res != 1] == P[res != 1]).all()
    # the families: inkala and hard1 have a solution, which a symmetry keeps; impossible has none
    assert (res[[0, 2]] == 1).all() and (res[3:27] == 1).all() and (res[51:75] == 1).all() and (res[[1] + list(range(27, 51))] != 1).all()
    for i in np.flatnonzero(res == 1):
        g = sol[i].reshape(9, 9)
        assert (g[P[i].reshape(9, 9) != 0] == P[i][P[i] != 0]).all()
        for unit in [g[r] for r in range(9)] + [g[:, c] for c in range(9)] + [g[r:r + 3, c:c + 3].reshape(9) for r in (0, 3, 6) for c in (0, 3, 6)]:
            assert sorted(unit.tolist()) == list(range(1, 10))
    # where oracle/_ref is built: the reference library itself, live, on the puzzles it finishes (it has no budget: not the ones that
    # spend 4096 nodes, the impossible seed among them); codes and solutions, it counts no nodes
    ref = os.path.join(ROOT, "oracle", "_ref", "libsudoku_ref.so")
    if os.path.exists(ref):
        ends = np.flatnonzero(res != 2)
        assert 1 not in ends
        codes, grids = sr._generator().solve_all(C.CDLL(ref), P[ends].reshape(-1, 9, 9).astype(np.int32))
        assert (codes == res[ends]).all() and (grids.reshape(-1, 81)[codes == 1] == sol[ends][codes == 1]).all()


def test_budget_is_a_prefix():
    """What expected_capped rests on: a run under a budget is the first nodes of a run under a larger one."""
    P = sr.puzzles_of("hard")
    for b in (1, 2, 9, 47, 48, 49):
        want = sr.expected_capped("hard", sr.HARD_CAP, b)
        rows = [sr.solve(p, b) for p in P]
        assert ([r[0] for r in rows] == want[0]).all() and ([r[2] for r in rows] == want[2]).all(), b
        assert (np.stack([r[1] for r in rows]) == want[1]).all(), b


def same_as(got, want, what):
    assert got[0].dtype == np.int8 and got[1].dtype == np.uint8 and got[2].dtype == np.int32
    for name, a, b in zip(("result", "solution", "nodes"), got, want):
        a = a.reshape(b.shape)
        bad = sorted({int(i[0]) for i in np.argwhere(a != b)})
        assert not bad, f"{what}: {name} differs in puzzles {bad[:8]}: got {a[bad[0]].tolist()} want {b[bad[0]].tolist()}"


def test_host_batch_matches_the_restatement_on_the_hard_set(host):
    """At the default budget and at the budgets on either side of the node where a search ends by itself: with k nodes the puzzle is
    solved or refuted in exactly k (the last node spent on the last failing leaf is NOSOLUTION, not BUDGET), with k - 1 it is BUDGET."""
    P = sr.hard_set()
    cap = sr.capped("hard", sr.HARD_CAP)
    edges = sr.edge_cases(cap[0], cap[2])
    budgets = sr.edge_budgets(cap[0], cap[2])
    print("edge cases:", edges, "budgets:", budgets)
    assert [name for name, _, _ in edges] == ["refuted0", "refuted1", "most", "fewest", "inkala"]
    assert all(b in budgets for _, _, k in edges for b in (k, k - 1)) and all(b in budgets for b in (48, 49, 256, 1024))
    for b in (sr.HARD_CAP,) + budgets:
        want = sr.expected_capped("hard", sr.HARD_CAP, b)
        got = {threads: host.solve_sudoku_batch(P, max_nodes=b, threads=threads) for threads in (1, 16)}
        for threads in (1, 16):
            same_as(got[threads], want, f"hard set, max_nodes={b}, threads={threads}")
        for name, i, k in edges:
            for res, sol, nodes in got.values():
                sol = sol.reshape(-1, 81)
                if b == k:
                    assert (res[i], nodes[i]) == (cap[0][i], k) and res[i] != sr.BUDGET and (sol[i] == cap[1][i]).all(), (name, b)
                if b == k - 1:
                    assert (res[i], nodes[i]) == (sr.BUDGET, k - 1) and (sol[i] == P[i]).all(), (name, b)


def test_host_matches_the_restatement_at_the_largest_budget(host):
    """The `impossible` seed alone under the 65536 nodes that are the device entry's largest budget (some 25 s of restatement)."""
    p = sr.hard_set()[1:2]
    want = sr.solve(p[0], 65536)
    got = host.solve_sudoku_batch(p, max_nodes=65536, threads=1)
    print("impossible at 65536: (result, nodes, depth, most levels left at once, entries after a return) =", (want[0],) + want[2:4] + want[5:])
    assert (int(got[0][0]), int(got[2][0])) == (want[0], want[2]) and (got[1].reshape(81) == want[1]).all()
    assert want[0] in (sr.NOSOLUTION, sr.BUDGET) and (want[1] == p[0]).all()


def test_host_batch_active_and_empty_and_arguments(host):
    P = sr.sparse_set()[:16]
    active = np.arange(16) % 3 != 1
    res, sol, nodes = host.solve_sudoku_batch(P, active=active, threads=4)
    full = host.solve_sudoku_batch(P, threads=4)
    assert (res[~active] == sr.SKIPPED).all() and (nodes[~active] == 0).all() and (sol.reshape(-1, 81)[~active] == P[~active]).all()
    for got, want in zip((res, sol, nodes), full):
        assert (got[active] == want[active]).all()
    res, sol, nodes = host.solve_sudoku_batch(np.zeros((0, 81), np.uint8))
    assert res.shape == (0,) and sol.shape == (0, 9, 9) and nodes.shape == (0,)
    with pytest.raises(TypeError):
        host.solve_sudoku_batch(P.astype(np.int32))
    with pytest.raises(ValueError):
        host.solve_sudoku_batch(P, max_nodes=-1)
    with pytest.raises(ValueError):
        host.solve_sudoku_batch(P, active=np.ones(3))


def test_single_entry_is_the_batch_of_one(host):
    for p, r, s in zip(sr.sparse_set()[:32], *sr.unbounded("sparse")[:2]):
        code, sol = host.solve_sudoku(p)
        assert code == r and (sol.reshape(81) == s).all()


