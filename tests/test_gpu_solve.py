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
