"""GPU: sv_solve_sudoku_batch (csrc/k14_solve.hip) through Context.solve_sudoku == the reference library's recorded answers
(tests/golden/solver_golden*.npz) and == the host batch entry (host.solve_sudoku_batch, itself checked against the plain-Python
restatement in tests/test_solve_ref.py) in result, solution and node count at every budget; then the layers above it:
FramePipeline(solve=True) and recognize_image(solve=True)."""
import os

import numpy as np
import pytest
import torch

import solve_ref as sr

pytestmark = pytest.mark.gpu


def run(ctx, grids, active=None, max_nodes=4096):
    """Context.solve_sudoku on host arrays, one launch -> (result, solution [n,81], nodes) as host arrays."""
    dev = ctx.solve_sudoku(torch.from_numpy(np.ascontiguousarray(grids)).to(ctx.device),
                           None if active is None else torch.from_numpy(active).to(ctx.device), max_nodes)
    assert set(dev) == {"solution", "result", "nodes"}
    assert dev["solution"].dtype == torch.uint8 and dev["result"].dtype == torch.int8 and dev["nodes"].dtype == torch.int32
    return dev["result"].cpu().numpy(), dev["solution"].cpu().numpy(), dev["nodes"].cpu().numpy()


def same(got, want, what):
    for name, a, b in zip(("result", "solution", "nodes"), got, want):
        b = b.reshape(a.shape)
        if not (a == b).all():
            bad = sorted({int(i[0]) for i in np.argwhere(a != b)})
            raise AssertionError(f"{what}: {name} differs in {len(bad)} frames, first {bad[:8]}: got {a[bad[0]].tolist()} want {b[bad[0]].tolist()}")


def host_batch(grids, active=None, max_nodes=0):
    import sudoku_vision_amd as sva
    return sva.host.solve_sudoku_batch(grids, active=active, max_nodes=max_nodes, threads=16)


def test_goldens_in_one_launch(ctx):
    """All 280 puzzles the reference library's answers are recorded for; entries outside a byte are clipped to 255 and stay invalid."""
    sets = sr.goldens()
    P = sr.as_bytes(np.concatenate([p.reshape(-1, 81) for _, p, _, _ in sets]))
    codes = np.concatenate([c for _, _, c, _ in sets])
    sols = np.concatenate([s.reshape(-1, 81) for _, _, _, s in sets])
    assert len(P) == 280
    res, sol, nodes = run(ctx, P)
    assert (res == codes).all()
    solved = codes == 1
    assert (sol[solved] == sols[solved]).all() and (sol[~solved] == P[~solved]).all()
    assert (nodes[codes == -1] == 0).all() and (nodes[codes != -1] >= 1).all()
    same((res, sol, nodes), host_batch(P), "goldens against the host")


@pytest.mark.parametrize("max_nodes", sr.BUDGETS)
def test_sparse_set_matches_the_host_at_every_budget(ctx, max_nodes):
    """Budget 0 is the host's `none`: the device is then given its default, which the condition of tests/test_solve_ref.py says no frame
    of this set spends."""
    P = sr.sparse_set()
    want = host_batch(P, max_nodes=max_nodes)
    got = run(ctx, P, max_nodes=max_nodes or 4096)
    same(got, want, f"sparse set, max_nodes={max_nodes}")
    spent = want[0] == sr.BUDGET
    assert spent.any() == (max_nodes in (1, 8))
    assert (got[2][spent] == max_nodes).all() and (got[1][spent] == P[spent]).all()


def test_crafted_cases_in_one_launch(ctx):
    names, grids = sr.crafted()
    P = np.concatenate([grids, sr.sparse_set()[sr.backtracking_case()][None]])
    names = names + ["backtracking"]
    res, sol, nodes = run(ctx, P)
    same((res, sol, nodes), host_batch(P), "crafted cases")
    got = {n: (int(r), int(k)) for n, r, k in zip(names, res, nodes)}
    assert got["empty"][0] == 1 and got["empty"][1] > 1
    assert got["full"] == (1, 1) and (sol[names.index("full")] == P[names.index("full")]).all()
    assert got["full_duplicate"] == (-1, 0) and got["value_10"] == (-1, 0)
    assert got["peers_same_sole_candidate"] == (0, 1) and got["two_digits_one_cell"] == (0, 1)
    want = sr.solve(P[-1])
    assert got["backtracking"] == (1, want[2]) and want[2] > want[3] and (sol[-1] == want[1]).all()
    for i in np.flatnonzero(res != 1):
        assert (sol[i] == P[i]).all()


def test_active_skips_frames_and_leaves_their_neighbours(ctx):
    P = sr.sparse_set()[:96]
    active = (np.arange(96) % 3 != 1).astype(np.uint8)
    res, sol, nodes = run(ctx, P, active=active)
    full = run(ctx, P)
    off = active == 0
    assert (res[off] == sr.SKIPPED).all() and (nodes[off] == 0).all() and (sol[off] == P[off]).all()
    for a, b in zip((res, sol, nodes), full):
        assert (a[~off] == b[~off]).all()
    same((res, sol, nodes), host_batch(P, active=active), "active against the host")
    same(run(ctx, P, active=active.astype(bool)), (res, sol, nodes), "a bool mask")


def test_sizes(ctx):
    res, sol, nodes = run(ctx, np.zeros((0, 81), np.uint8))
    assert res.shape == (0,) and sol.shape == (0, 81) and nodes.shape == (0,)
    P = sr.sparse_set()
    same(run(ctx, P[4:5]), host_batch(P[4:5]), "n = 1")
    tail = np.concatenate([P[:256], P[300:301]])                        # n = 257: the last frame is a workgroup of its own kind
    assert (tail[256] != tail[0]).any()
    same(run(ctx, tail), host_batch(tail), "n = 257")


def test_out_tensors_partial_out_and_argument_ranges(ctx):
    P = torch.from_numpy(sr.sparse_set()[:64]).to(ctx.device)
    want = ctx.solve_sudoku(P)
    outs = {"solution": torch.full((64, 81), 77, dtype=torch.uint8, device=ctx.device), "result": torch.full((64,), 77, dtype=torch.int8, device=ctx.device),
            "nodes": torch.full((64,), -7, dtype=torch.int32, device=ctx.device)}
    got = ctx.solve_sudoku(P, out=outs)
    assert all(got[k] is outs[k] and torch.equal(outs[k], want[k]) for k in outs)
    for keys in (("result",), ("nodes", "solution"), ()):
        part = {k: torch.full_like(want[k], 77) for k in keys}
        got = ctx.solve_sudoku(P, out=part)
        assert set(got) == set(keys) and all(got[k] is part[k] and torch.equal(part[k], want[k]) for k in keys)
    again = ctx.solve_sudoku(P)
    assert all(torch.equal(again[k], want[k]) for k in want)                # two launches, one answer
    import sudoku_vision_amd as sva
    for bad in (0, 65537, -1):
        with pytest.raises(sva._native.NativeError, match="SV_ERR_BAD_ARG"):
            ctx.solve_sudoku(P, max_nodes=bad)
    same([t.cpu().numpy() for t in (lambda d: (d["result"], d["solution"], d["nodes"]))(ctx.solve_sudoku(P, max_nodes=65536))],
         [want[k].cpu().numpy() for k in ("result", "solution", "nodes")], "the largest budget")
    with pytest.raises(KeyError):
        ctx.solve_sudoku(P, out={"grid": want["solution"]})
    with pytest.raises(TypeError):
        ctx.solve_sudoku(P, out={"result": torch.empty((64,), dtype=torch.int32, device=ctx.device)})
    with pytest.raises(ValueError):
        ctx.solve_sudoku(P, active=torch.ones((3,), dtype=torch.uint8, device=ctx.device))
    with pytest.raises(TypeError):
        ctx.solve_sudoku(P.cpu())


# ---- the hard set (tests/solve_ref.py): searches that go deep, leave several levels at once, reuse levels, refute late or spend 4096 ------
def _hard_edges():
    """The host's run of the hard set at the default budget (tests/test_solve_ref.py holds it to the restatement) and the budgets on
    either side of the nodes where its searches end: the restatement's own run takes the better part of a minute, this one a moment."""
    res, _, nodes = host_batch(sr.hard_set(), max_nodes=sr.HARD_CAP)
    return sr.edge_cases(res, nodes), sr.edge_budgets(res, nodes)


HARD_EDGES, EDGE_BUDGETS = _hard_edges()


def test_hard_set_matches_the_host_at_the_default_budget(ctx):
    P = sr.hard_set()
    want = host_batch(P, max_nodes=4096)
    got = run(ctx, P, max_nodes=4096)
    same(got, want, "hard set, max_nodes=4096")
    res, sol, nodes = got
    assert set(res.tolist()) == {0, 1, 2}
    spent = res == sr.BUDGET
    assert (nodes[spent] == 4096).all() and (sol[spent] == P[spent]).all() and (sol[res == 0] == P[res == 0]).all()
    assert ((res == 0) & (nodes > 1000)).sum() >= 2 and spent.sum() >= 10


@pytest.mark.parametrize("max_nodes", EDGE_BUDGETS)
def test_hard_set_matches_the_host_at_edge_budgets(ctx, max_nodes):
    """With the k nodes its search takes a puzzle is solved or refuted in exactly k: the last node spent on the last failing leaf is
    NOSOLUTION, not BUDGET.  With k - 1 it is BUDGET."""
    P = sr.hard_set()
    want = host_batch(P, max_nodes=max_nodes)
    got = run(ctx, P, max_nodes=max_nodes)
    same(got, want, f"hard set, max_nodes={max_nodes}")
    res, sol, nodes = got
    spent = res == sr.BUDGET
    assert spent.any() and (nodes[spent] == max_nodes).all() and (sol[spent] == P[spent]).all()
    full = host_batch(P, max_nodes=sr.HARD_CAP)
    for name, i, k in HARD_EDGES:
        if max_nodes == k:
            assert (res[i], nodes[i]) == (full[0][i], k) and res[i] != sr.BUDGET and (sol[i] == full[1].reshape(-1, 81)[i]).all(), name
        if max_nodes == k - 1:
            assert (res[i], nodes[i]) == (sr.BUDGET, k - 1) and (sol[i] == P[i]).all(), name


def test_hard_and_easy_and_skipped_share_a_launch(ctx):
    """Hard, sparse and crafted frames interleaved, every fifth switched off: a frame's answer does not depend on its neighbours, not
    even on one that runs 4096 nodes beside it."""
    names, grids = sr.crafted()
    hard, easy = sr.hard_set(), sr.sparse_set()[:75]
    P = np.empty((150, 81), np.uint8)
    P[0::2], P[1::2] = hard, easy
    P = np.concatenate([P[:77], grids, P[77:]])                          # the crafted cases in the middle: 75 + 75 + 6 frames
    n = len(P)
    assert n == 150 + len(names) and n % 64 and n % 5
    active = (np.arange(n) % 5 != 2).astype(np.uint8)
    is_hard = np.zeros(n, bool)
    is_hard[:77:2] = True
    is_hard[77 + len(names) + 1::2] = True
    assert is_hard.sum() == 75 and (P[is_hard] == hard).all()
    off = active == 0
    assert (off & is_hard).sum() >= 10 and (off & ~is_hard).sum() >= 10
    got = run(ctx, P, active=active)
    same(got, host_batch(P, active=active, max_nodes=4096), "hard, easy and skipped frames in one launch")
    res, sol, nodes = got
    assert (res[off] == sr.SKIPPED).all() and (nodes[off] == 0).all() and (sol[off] == P[off]).all()
    alone = run(ctx, P)
    for a, b in zip(got, alone):
        assert (a[~off] == b[~off]).all()
    long = np.flatnonzero((nodes == 4096) & (res == sr.BUDGET))
    assert len(long) >= 10
    each = host_batch(P, max_nodes=4096)                                 # every frame's own answer, nothing switched off
    for i in long:
        for j in (i - 1, i + 1):
            if 0 <= j < n and not off[j]:
                assert res[j] == each[0][j] and nodes[j] == each[2][j] and (sol[j] == each[1].reshape(-1, 81)[j]).all(), (i, j)


def test_two_launches_of_the_hard_set_agree(ctx):
    """A stack level left over from the launch before, or from the frame a workgroup's LDS held before, changes nothing."""
    P = torch.from_numpy(sr.hard_set()).to(ctx.device)
    runs = []
    for _ in range(2):
        out = {"solution": torch.full((75, 81), 77, dtype=torch.uint8, device=ctx.device),
               "result": torch.full((75,), 77, dtype=torch.int8, device=ctx.device),
               "nodes": torch.full((75,), 77, dtype=torch.int32, device=ctx.device)}
        got = ctx.solve_sudoku(P, None, 4096, out)
        assert all(got[k] is out[k] for k in out)
        runs.append(tuple(out[k].cpu().numpy() for k in ("result", "solution", "nodes")))
    same(runs[1], runs[0], "the second launch against the first")
    same(runs[0], host_batch(sr.hard_set(), max_nodes=4096), "out= against the host")
    assert not (runs[0][0] == 77).any()                                 # (77 is a node count the set has: the host comparison covers nodes)


def test_hard_frames_at_the_largest_budget(ctx):
    """`impossible` and its first two morphs under the entry's largest budget of 65536 nodes.  One wave runs one puzzle, so the launch
    is as long as its slowest frame: 178.5 ms of wall time on an MI355X for the launch with its copies (two frames spend all 65536
    nodes, some 2.7 µs per node; the first morph is refuted after 3842).  The limit of 10 s below is the one past which this test
    would have had to go down to 16384 nodes."""
    import time
    P = sr.hard_set()[[1, 27, 28]]
    want = host_batch(P, max_nodes=65536)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = run(ctx, P, max_nodes=65536)
    wall = time.perf_counter() - t0
    print(f"K14, 3 frames at max_nodes=65536: {wall * 1e3:.1f} ms; result {got[0].tolist()} nodes {got[2].tolist()}")
    same(got, want, "the impossible family, max_nodes=65536")
    assert (got[0] != 1).all() and (got[2] > 4096).sum() >= 2 and (got[1] == P).all()
    assert wall < 10.0


# ---- the pipeline: the batch of tests/test_gpu_propagate.py, whose recognised logits are replaced by chosen ones --------------------------
@pytest.fixture(scope="module")
def pool(golden_dir):
    import constraint_ref as cr
    import test_gpu_propagate as tp
    golden = np.load(os.path.join(golden_dir, "constraint_goldens.npz"))
    read, second, _ = tp._pool((cr.frames()[0],), golden)
    return tp, read, second


def test_frame_pipeline_solve(ctx, monkeypatch, pool):
    """Frame f is read as kind f % 4 of test_gpu_propagate._pool; frame 5 is blank: no grid."""
    from sudoku_vision_amd.pipeline import FramePipeline
    from sudoku_vision_amd.synth import synth_frames, random_state_dict
    tp, read, second = pool
    ctx.load_state_dict(random_state_dict(1234))
    n, H, W = 24, 270, 480
    frames, _, _ = synth_frames(n, H, W, seed=17, device="cuda")
    frames = frames.contiguous()
    frames[5] = 0
    crafted = torch.from_numpy(np.stack([tp._logits(read[f], second[f]) for f in range(n)])).to(ctx.device)
    torch.cuda.synchronize()
    tp._inject(monkeypatch, ctx, crafted, frames)
    keys = {"solution", "solve_result", "solve_nodes"}
    seen = set()
    for resolve in (False, True):
        for propagate in (False, True):
            off_p = FramePipeline(ctx, H, W, chunk=8, depth=3, resolve=resolve, propagate=propagate)
            on_p = FramePipeline(ctx, H, W, chunk=8, depth=3, resolve=resolve, propagate=propagate, solve=True)
            off, on = off_p.run(frames), on_p.run(frames)
            assert set(on) - set(off) == keys
            for key in off:
                a, b = off[key], on[key]
                assert torch.equal(a, b) if isinstance(a, torch.Tensor) else (a == b).all(), key
            assert off_p.describe() != on_p.describe() and "K14" in on_p.describe() and "K14" not in off_p.describe()
            found = on["found"]
            assert not found[5] and found.sum() == n - 1
            given = on["propagated_digits" if propagate else "resolved_digits" if resolve else "digits"].cpu().numpy()
            active = on["propagate_valid"].cpu().numpy() if propagate else found
            want = host_batch(given, active=active, max_nodes=4096)
            got = (on["solve_result"].cpu().numpy(), on["solution"].cpu().numpy(), on["solve_nodes"].cpu().numpy())
            assert on["solve_result"].dtype == torch.int8 and on["solution"].dtype == torch.uint8 and on["solve_nodes"].dtype == torch.int32
            same(got, want, f"pipeline resolve={resolve} propagate={propagate}")
            assert got[0][5] == sr.SKIPPED and not got[1][5].any() and got[2][5] == 0
            assert (got[0][found & (np.arange(n) % 4 == 0)] == 1).all()                    # a consistent grid is solved
            seen |= set(got[0].tolist())
    assert {1, sr.SKIPPED} <= seen
    # a budget of one node: the frames that need a second one are reported, not finished
    small = FramePipeline(ctx, H, W, chunk=8, depth=3, solve=True, solve_max_nodes=1).run(frames)
    want = host_batch(small["digits"].cpu().numpy(), active=small["found"], max_nodes=1)
    same((small["solve_result"].cpu().numpy(), small["solution"].cpu().numpy(), small["solve_nodes"].cpu().numpy()), want, "pipeline, one node")


def test_recognize_image_solve(ctx, golden_dir, monkeypatch, pool):
    from sudoku_vision_amd import imgcodecs
    from sudoku_vision_amd.pipeline import recognize_image, run_solver
    from sudoku_vision_amd.synth import random_state_dict
    tp, read, second = pool
    sd = random_state_dict(99)
    img = imgcodecs.imread(os.path.join(golden_dir, "sample_1.jpg"))
    # what the recogniser reads: the sparse set's backtracking puzzle (it needs more than one node), then the pool's kinds
    hard = sr.sparse_set()[sr.backtracking_case()]
    for f, (grid, alt) in enumerate([(hard, {})] + [(read[k], second[k]) for k in (0, 1, 2)]):
        tp._inject(monkeypatch, ctx, torch.from_numpy(tp._logits(grid, alt)).to(ctx.device)[None])
        for resolve, propagate in ((False, False), (True, False), (False, True), (True, True)):
            base = recognize_image(img, sd, ctx=ctx, resolve=resolve, propagate=propagate)
            res = recognize_image(img, sd, ctx=ctx, resolve=resolve, propagate=propagate, solve=True)
            assert set(res) - set(base) == {"solve_result", "solution", "solve_nodes"}
            for key in base:
                assert np.array_equal(np.asarray(res[key], dtype=object), np.asarray(base[key], dtype=object)), key
            given = res["propagated_grid"] if propagate else res["resolved_grid"] if resolve else res["grid"]
            if propagate and not res["propagation"]["is_valid"]:
                assert (res["solve_result"], res["solution"], res["solve_nodes"]) == (sr.SKIPPED, given, 0)
                continue
            ok, solution = run_solver(given)
            assert res["solution"] == solution and (res["solve_result"] == 1) == ok
            code, _, nodes = host_batch(np.array(given, np.uint8).reshape(1, 81))
            assert res["solve_result"] == code[0] and res["solve_nodes"] == nodes[0]
    # the device's budget forced down to one node: the frame ends there with result 2 and the host finishes it, same answer
    tp._inject(monkeypatch, ctx, torch.from_numpy(tp._logits(hard)).to(ctx.device)[None])
    want = recognize_image(img, sd, ctx=ctx, solve=True)
    assert want["solve_result"] == 1 and want["solve_nodes"] > 1
    real, seen = ctx.solve_sudoku, []

    def one_node(digits, active=None, max_nodes=4096, out=None):
        r = real(digits, active, 1, out)
        seen.append(int(r["result"][0]))
        return r
    monkeypatch.setattr(ctx, "solve_sudoku", one_node)
    res = recognize_image(img, sd, ctx=ctx, solve=True)
    assert seen == [sr.BUDGET]
    assert (res["solve_result"], res["solution"], res["solve_nodes"]) == (want["solve_result"], want["solution"], want["solve_nodes"])
