"""GPU: sv_propagate_constraints (csrc/k10_propagate.hip) through Context.propagate_constraints == the plain-Python restatement
(tests/constraint_ref.py) == the reference's own results (tests/golden/constraint_goldens.npz), every output byte for byte; then the
layers above it: the resolve/constraint_resolver.py drop-in, recognize_image(propagate=True) and FramePipeline(propagate=True)."""
import os
import sys

import numpy as np
import pytest
import torch

import constraint_ref as cr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "constraint_goldens.npz"))


@pytest.fixture(scope="module")
def generated():
    """The 512 generated frames and the restatement's results for them, computed once."""
    digits, conf = cr.frames()
    return digits, conf, cr.propagate(digits, conf)


def run(ctx, digits, conf=None, max_iterations=100, batch=None):
    """Context.propagate_constraints on host arrays, in launches of `batch` frames -> host arrays."""
    n = digits.shape[0]
    batch = batch or max(n, 1)
    dd = torch.from_numpy(digits).to(ctx.device)
    dc = None if conf is None else torch.from_numpy(conf).to(ctx.device)
    parts = [ctx.propagate_constraints(dd[s:s + batch], None if dc is None else dc[s:s + batch], max_iterations) for s in range(0, max(n, 1), batch)]
    got = {key: torch.cat([p[key] for p in parts]).cpu().numpy() for key in cr.FIELDS}
    got["candidates"] = got["candidates"].view(np.uint16)
    return got


def same(got, want, what, rows=None):
    for key in cr.FIELDS:
        a, b = got[key], want[key] if rows is None else want[key][rows]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = sorted({int(i[0]) for i in np.argwhere(a != b)})
            raise AssertionError(f"{what}: {key} differs in {len(bad)} frames, first {bad[:8]}: got {a[bad[0]].tolist()} want {b[bad[0]].tolist()}")


def from_golden(golden, prefix):
    return {key: golden[f"{prefix}.{key}"] for key in cr.FIELDS}


def test_generated_frames_one_batch(ctx, generated, golden):
    digits, conf, want = generated
    got = run(ctx, digits, conf)
    same(got, want, "512 frames, one launch")
    same(got, from_golden(golden, "gen"), "512 frames against the reference's results")


@pytest.mark.parametrize("batch", [1, 5])
def test_generated_frames_small_batches(ctx, generated, batch):
    """Launches of 1 and of 5 frames; every tenth frame is enough for launches of 1 to meet every kind."""
    digits, conf, want = generated
    rows = np.arange(0, digits.shape[0], 10 if batch == 1 else 1)
    same(run(ctx, digits[rows], conf[rows], batch=batch), want, f"launches of {batch}", rows)


def test_result_does_not_depend_on_the_batch(ctx, generated):
    digits, conf, want = generated
    rows = np.arange(cr.PER_KIND, digits.shape[0])
    same(run(ctx, digits[rows], conf[rows]), want, "consistent frames removed", rows)


@pytest.mark.parametrize("name", sorted(cr.crafted_cases()))
def test_crafted_case(ctx, golden, name):
    digits, conf, it = cr.crafted_cases()[name]
    got = run(ctx, digits, conf, it)
    same(got, cr.propagate(digits, conf, it), name)
    same(got, from_golden(golden, f"case.{name}"), f"{name} against the reference's result")


def test_argument_ranges_empty_batch_and_bytes_that_are_no_digits(ctx, generated):
    import sudoku_vision_amd as sva
    digits, conf, want = generated
    dd = torch.from_numpy(digits[:4]).to(ctx.device)
    for it in (0, -1, 101):
        with pytest.raises(sva._native.NativeError, match="SV_ERR_UNSUPPORTED"):
            ctx.propagate_constraints(dd, max_iterations=it)
    empty = ctx.propagate_constraints(dd[:0])
    assert empty["grid"].shape == (0, 81) and empty["resolved"].shape == (0, 81, 2) and empty["iterations"].shape == (0,)
    with pytest.raises(TypeError):
        ctx.propagate_constraints(dd.to(torch.int32))
    with pytest.raises(ValueError):
        ctx.propagate_constraints(dd[:, :80])
    # frames 1 and 3 hold a byte above 9 (in a lane's first and in its second cell): no grid; their neighbours are untouched
    broken = digits[:5].copy()
    broken[1, 7], broken[3, 80] = 10, 255
    got = run(ctx, broken, conf[:5])
    same(got, cr.propagate(broken, conf[:5]), "bytes above 9")
    for f in (1, 3):
        assert (got["is_valid"][f], got["iterations"][f], got["contradiction_cell"][f], got["n_resolved"][f]) == (0, 0, 255, 0)
        assert (got["grid"][f] == broken[f]).all() and not got["candidates"][f].any()
    for f in (0, 2, 4):
        assert all(got[key][f].tobytes() == want[key][f].tobytes() for key in cr.FIELDS)


def test_out_tensors_are_written_in_place(ctx, generated):
    digits, conf, want = generated
    rows = np.arange(100, 140)                                      # consistent and misread frames
    dd, dc = torch.from_numpy(digits[rows]).to(ctx.device), torch.from_numpy(conf[rows]).to(ctx.device)
    grid = torch.full((48, 81), 77, dtype=torch.uint8, device=ctx.device)
    res = torch.full((48, 81, 2), 77, dtype=torch.uint8, device=ctx.device)
    cand = torch.full((48, 81), 77, dtype=torch.int16, device=ctx.device)
    nres = torch.full((40,), 77, dtype=torch.uint8, device=ctx.device)
    got = ctx.propagate_constraints(dd, dc, out={"grid": grid[4:44], "resolved": res[4:44], "candidates": cand[4:44], "n_resolved": nres})
    assert set(got) == {"grid", "resolved", "candidates", "n_resolved"} and got["n_resolved"] is nres
    for t, key in ((grid, "grid"), (res, "resolved"), (cand, "candidates")):
        assert (t[4:44].cpu().numpy().view(want[key].dtype) == want[key][rows]).all(), key
        assert (t[:4] == 77).all() and (t[44:] == 77).all(), key
    assert (nres.cpu().numpy() == want["n_resolved"][rows]).all()
    same_grid = dd.clone()                                          # grid may be digits itself
    ctx.propagate_constraints(same_grid, out={"grid": same_grid})
    assert (same_grid.cpu().numpy() == want["grid"][rows]).all()
    with pytest.raises(TypeError):
        ctx.propagate_constraints(dd, out={"grid": grid})
    with pytest.raises(TypeError):
        ctx.propagate_constraints(dd, out={"candidates": grid[4:44]})
    with pytest.raises(KeyError):
        ctx.propagate_constraints(dd, out={"digits": grid[4:44]})


# ---- the drop-in module ---------------------------------------------------------------------------------------------------------------
def _dropin():
    d = os.path.join(ROOT, "sudoku-vision_amd", "resolve")
    if d not in sys.path:
        sys.path.insert(0, d)
    import constraint_resolver
    assert os.path.dirname(os.path.abspath(constraint_resolver.__file__)) == d
    return constraint_resolver


def _check_dropin(mod, digits, conf, g, f):
    grid = [[int(v) for v in row] for row in digits.reshape(9, 9)]
    c = None if conf is None else [[float(v) for v in row] for row in conf.reshape(9, 9)]
    solver = mod.ConstraintResolver(grid, c)
    res = solver.propagate()
    n = int(g["n_resolved"][f])
    bad = int(g["contradiction_cell"][f])
    assert isinstance(res, mod.PropagationResult) and res.grid == g["grid"][f].reshape(9, 9).tolist()
    assert (res.is_valid, res.iterations) == (bool(g["is_valid"][f]), int(g["iterations"][f]))
    assert res.contradiction_cell == (None if bad == cr.NONE else (bad // 9, bad % 9))
    assert res.cells_resolved == [(int(x) // 9, int(x) % 9, int(v)) for x, v in g["resolved"][f][:n]]
    assert len(res.cells) == 81
    for x, cell in enumerate(res.cells):
        assert isinstance(cell, mod.Cell) and (cell.row, cell.col, cell.value) == (x // 9, x % 9, int(g["grid"][f][x]))
        assert cell.candidates == {d for d in range(1, 10) if int(g["candidates"][f][x]) >> d & 1} == solver.get_candidates(x // 9, x % 9)
        assert cell.is_fixed == bool(g["is_fixed"][f][x]) and cell.confidence == (1.0 if c is None else c[x // 9][x % 9])
    with pytest.raises(RuntimeError):
        solver.propagate()
    return res


def test_dropin_module_on_the_selftest_and_generated_frames(ctx, golden, generated):
    mod = _dropin()
    digits, conf, _ = generated
    res = _check_dropin(mod, np.array(cr.SELFTEST, np.uint8), None, from_golden(golden, "case.selftest"), 0)
    assert res.is_valid and len(res.cells_resolved) == 51 and all(v for row in res.grid for v in row)
    plain = mod.resolve_with_constraints(cr.SELFTEST)
    assert (plain.grid, plain.cells_resolved, plain.iterations) == (res.grid, res.cells_resolved, res.iterations)
    differs = np.nonzero(golden["gen.order_differs"])[0]
    rows = [0, 1, 2] + [int(f) for f in differs[:2]] + [int(f) for f in np.nonzero(golden["gen.valid_differs"])[0][:1]] + [300, 450]
    assert len(rows) == 8
    for f in rows:
        _check_dropin(mod, digits[f], conf[f], from_golden(golden, "gen"), f)
    with pytest.raises(ValueError):
        mod.ConstraintResolver([[10] * 9] * 9)


# ---- the pipeline: recognised logits are replaced by chosen ones where the CNN hands them over ------------------------------------------
def _logits(read, second=None):
    """Logits [81,10] of a recogniser that reads `read` (top-1 0.9996); second: {cell: digit} cells read unsurely (0.62) with that
    digit as the runner-up (0.38)."""
    logits = np.full((81, 10), -4.0, np.float32)
    logits[np.arange(81), read] = 6.0
    for x, d in (second or {}).items():
        logits[x] = -4.0
        logits[x, read[x]], logits[x, d] = 3.0, 2.5
    return logits


def _inject(monkeypatch, ctx, crafted, frames=None):
    """ctx.frames_to_digits runs as it is and then hands over `crafted` logits [n,81,10] (device) instead of its own: those of the
    frames it was given, found by their address in `frames` (None: the one frame of a single call)."""
    real = ctx.frames_to_digits

    def fake(chunk, minv, out=None, **kw):
        r = real(chunk, minv, out=out, **kw)
        s = 0 if frames is None else (chunk.data_ptr() - frames.data_ptr()) // frames[0].numel()
        mine = crafted[s:s + chunk.shape[0]]
        r["logits"].copy_(mine)
        r["digits"].copy_(mine.argmax(-1).to(torch.uint8))
        r["conf"].copy_(torch.softmax(mine, -1).max(-1).values)
        return r
    monkeypatch.setattr(ctx, "frames_to_digits", fake)


def _pool(generated, golden):
    """Frames to read, by kind: 0 a consistent grid; 1 a consistent grid with one cell misread as a shown peer's digit, the truth its
    runner-up (K9 repairs it); 2 a generated frame whose propagation ends in a contradiction; 3 a generated frame on which the
    hidden singles' order decides the outcome.  -> (read [n,81], second: list of {cell: digit}, repaired [n,81])"""
    digits = generated[0]
    contradictory = [int(f) for f in np.nonzero(golden["gen.is_valid"] == 0)[0] if not _conflicts(digits[f])]
    ordered = [int(f) for f in np.nonzero(golden["gen.order_differs"])[0] if not _conflicts(digits[f])]
    assert len(contradictory) >= 6 and len(ordered) >= 6
    read, second, repaired = [], [], []
    for f in range(24):
        kind = f % 4
        base = digits[(f, f, contradictory[f // 4], ordered[f // 4])[kind]].copy()
        good, alt = base.copy(), {}
        if kind == 1:
            x = next(x for x in range(81) if base[x] and any(base[y] and base[y] != base[x] for y in cr.PEERS[x]))
            alt = {x: int(base[x])}
            base[x] = next(base[y] for y in cr.PEERS[x] if base[y] and base[y] != base[x])
        read.append(base)
        second.append(alt)
        repaired.append(good)
    return np.stack(read), second, np.stack(repaired)


def _conflicts(g):
    return any(len(v) != len(set(v)) for u in cr.UNITS for v in [[int(g[x]) for x in u if g[x]]])


def test_recognize_image_propagate(ctx, golden_dir, monkeypatch, generated, golden):
    from sudoku_vision_amd import imgcodecs
    from sudoku_vision_amd.pipeline import recognize_image
    from sudoku_vision_amd.synth import random_state_dict
    sd = random_state_dict(99)
    img = imgcodecs.imread(os.path.join(golden_dir, "sample_1.jpg"))
    read, second, repaired = _pool(generated, golden)
    for f in (0, 1, 2, 3):
        _inject(monkeypatch, ctx, torch.from_numpy(_logits(read[f], second[f])).to(ctx.device)[None])
        for resolve in (False, True):
            base = recognize_image(img, sd, ctx=ctx, resolve=resolve)
            res = recognize_image(img, sd, ctx=ctx, resolve=resolve, propagate=True)
            assert set(res) - set(base) == {"propagation", "propagated_grid"}
            for key in base:
                assert np.array_equal(np.asarray(res[key], dtype=object), np.asarray(base[key], dtype=object)), key
            start = np.array(res["resolved_grid"] if resolve else res["grid"], np.uint8).reshape(1, 81)
            assert (start[0] == (repaired[f] if resolve else read[f])).all()
            conf = torch.softmax(torch.from_numpy(_logits(read[f], second[f])), -1).numpy()
            conf = conf[np.arange(81), start[0]][None].astype(np.float32)
            want = cr.propagate(start, conf)
            bad, n = int(want["contradiction_cell"][0]), int(want["n_resolved"][0])
            assert res["propagated_grid"] == want["grid"][0].reshape(9, 9).tolist()
            assert res["propagation"] == {"is_valid": bool(want["is_valid"][0]), "iterations": int(want["iterations"][0]),
                                          "contradiction_cell": None if bad == cr.NONE else (bad // 9, bad % 9),
                                          "cells_resolved": [(int(x) // 9, int(x) % 9, int(v)) for x, v in want["resolved"][0][:n]]}
            if f == 2:
                assert not res["propagation"]["is_valid"] and res["propagation"]["contradiction_cell"] is not None
            if f < 2 and (resolve or f == 0):
                assert res["propagation"]["is_valid"] and res["propagation"]["cells_resolved"]


def test_frame_pipeline_propagate(ctx, monkeypatch, generated, golden):
    """Frame f of the pool is read as kind f % 4 of _pool; frame 5 is blank: no grid."""
    from sudoku_vision_amd.pipeline import FramePipeline
    from sudoku_vision_amd.synth import synth_frames, random_state_dict
    ctx.load_state_dict(random_state_dict(1234))
    n, H, W = 24, 270, 480
    frames, _, _ = synth_frames(n, H, W, seed=17, device="cuda")
    frames = frames.contiguous()
    frames[5] = 0
    read, second, repaired = _pool(generated, golden)
    crafted = torch.from_numpy(np.stack([_logits(read[f], second[f]) for f in range(n)])).to(ctx.device)
    torch.cuda.synchronize()
    _inject(monkeypatch, ctx, crafted, frames)
    keys = {"propagated_digits", "propagate_valid", "contradiction_cell", "n_propagated"}
    for resolve in (False, True):
        off_p = FramePipeline(ctx, H, W, chunk=8, depth=3, resolve=resolve)
        on_p = FramePipeline(ctx, H, W, chunk=8, depth=3, resolve=resolve, propagate=True)
        off, on = off_p.run(frames), on_p.run(frames)
        assert set(on) - set(off) == keys and on["propagate_valid"].dtype == torch.bool
        for key in off:
            a, b = off[key], on[key]
            assert torch.equal(a, b) if isinstance(a, torch.Tensor) else (a == b).all(), key
        assert off_p.describe() == FramePipeline(ctx, H, W, chunk=8, depth=3, resolve=resolve, propagate=False).describe() != on_p.describe()
        found = on["found"]
        assert not found[5] and found.sum() == n - 1
        start = on["resolved_digits" if resolve else "digits"].cpu().numpy()
        assert (start[found] == (repaired if resolve else read)[found]).all()
        want = cr.propagate(start)
        got = {key: on[key].cpu().numpy() for key in keys}
        for key, name in (("propagated_digits", "grid"), ("propagate_valid", "is_valid"), ("contradiction_cell", "contradiction_cell"), ("n_propagated", "n_resolved")):
            assert (got[key][found] == want[name][found]).all(), (resolve, key)
        assert not got["propagated_digits"][5].any() and not got["propagate_valid"][5] and got["contradiction_cell"][5] == 255 and got["n_propagated"][5] == 0
        kind = np.arange(n) % 4
        assert not got["propagate_valid"][found & (kind == 2)].any() and got["propagate_valid"][found & (kind == 0)].all()
        if resolve:
            assert got["propagate_valid"][found & (kind == 1)].all() and (on["n_corrections"].cpu().numpy()[found & (kind == 1)] == 1).all()
