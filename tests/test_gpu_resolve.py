"""GPU: sv_resolve_conflicts (csrc/k9_resolve.hip) through Context.resolve_conflicts == the plain-Python restatement
(tests/resolve_ref.py) == the reference's own results (tests/golden/resolve_goldens.npz), every output, the f64 score to the bit; then
the layers above it: the resolve/ drop-in modules, recognize_image(resolve=True) and FramePipeline(resolve=True).

The generated frames hold integers / 4096, whose sums are exact even in f32; the real-probability sets (resolve_ref.real_frames, the
thresholds of resolve_ref.MINALT) hold f32-rounded softmax outputs, on which a kernel that summed, averaged or compared in f32 differs
from the restatement (tests/test_resolve_ref.py shows it on mutants of the restatement); and the chain tests run K9 on what
k_softmax_topk itself returns.  All inside the domain in which the score is exact: confidences that enter a sum are >= 2^-18."""
import os
import sys

import numpy as np
import pytest
import torch

import resolve_ref as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "resolve_goldens.npz"))


@pytest.fixture(scope="module")
def generated():
    """The 512 generated frames and the restatement's results for them, computed once."""
    index, prob = rr.frames(rr.GOLDEN_SEED, rr.GOLDEN_N)
    return index, prob, rr.resolve(index, prob)


def run(ctx, index, prob, batch=None, **kw):
    """Context.resolve_conflicts on host arrays, in launches of `batch` frames -> host arrays."""
    n = index.shape[0]
    batch = batch or max(n, 1)
    di, dp = torch.from_numpy(index).to(ctx.device), torch.from_numpy(prob).to(ctx.device)
    parts = [ctx.resolve_conflicts(di[s:s + batch], dp[s:s + batch], **kw) for s in range(0, max(n, 1), batch)]
    return {key: torch.cat([p[key] for p in parts]).cpu().numpy() for key in rr.FIELDS}


def same(got, want, what, rows=None):
    for key in rr.FIELDS:
        a, b = got[key], want[key] if rows is None else want[key][rows]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = sorted({int(i[0]) for i in np.argwhere(a.view(np.uint64 if key == "score" else a.dtype) != b.view(np.uint64 if key == "score" else b.dtype))})
            raise AssertionError(f"{what}: {key} differs in {len(bad)} frames, first {bad[:8]}: got {a[bad[0]].tolist()} want {b[bad[0]].tolist()}")


def from_golden(golden, prefix):
    return {key: golden[f"{prefix}.{key}"] for key in rr.FIELDS}


def test_generated_frames_one_batch(ctx, generated, golden):
    index, prob, want = generated
    got = run(ctx, index, prob)
    same(got, want, "512 frames, one launch")
    same(got, from_golden(golden, "gen"), "512 frames against the reference's results")


@pytest.mark.parametrize("batch", [1, 5])
def test_generated_frames_small_batches(ctx, generated, batch):
    """Launches of 1 and of 5 frames: valid frames and searching frames side by side, and a last launch that is not full."""
    index, prob, want = generated
    same(run(ctx, index, prob, batch=batch), want, f"launches of {batch}")


def test_result_does_not_depend_on_the_batch(ctx, generated):
    index, prob, want = generated
    rows = np.nonzero(want["num_conflicts_before"] > 0)[0]
    assert 0 < rows.size < index.shape[0]
    same(run(ctx, index[rows], prob[rows]), want, "valid frames removed", rows)


@pytest.mark.parametrize("name", sorted(rr.crafted_cases()))
def test_crafted_case(ctx, golden, name):
    index, prob = rr.crafted_cases()[name]
    got = run(ctx, index, prob)
    same(got, rr.resolve(index, prob), name)
    same(got, from_golden(golden, f"case.{name}"), f"{name} against the reference's result")


def test_crafted_cases_show_what_they_are_for(ctx):
    """The rules the crafted frames were built around, spelled out on the kernel's results."""
    got = {name: run(ctx, *frame) for name, frame in rr.crafted_cases().items()}

    def one(name, key):
        return got[name][key][0].tolist()
    assert (one("valid", "success"), one("valid", "paths_explored"), one("valid", "n_corrections")) == (1, 1, 0)
    assert one("selftest", "corr_cells")[0] == [3, 5, 8] and one("selftest", "n_corrections") == 1 and one("selftest", "success") == 1
    assert (one("all_weak", "success"), one("all_weak", "paths_explored"), one("all_weak", "n_corrections")) == (0, 1, 0)
    assert (got["all_weak"]["index"] == rr.crafted_cases()["all_weak"][0]).all()
    assert one("count3", "num_conflicts_after") == 3 and one("count3", "conflict_count")[0] == 3
    assert one("three_in_row_weak", "num_conflicts_before") == 1 and sum(one("three_in_row_weak", "conflict_count")) == 3
    assert one("tie_first_named", "corr_cells")[0] == [0, 5, 1] and one("tie_first_named", "paths_explored") == 2
    assert [c[0] for c in one("named_order_two", "corr_cells")[:2]] == [45, 12]          # (5,0) is named before (1,3)
    assert (one("exact_two", "n_corrections"), one("exact_three", "n_corrections")) == (2, 3)
    assert (one("exact_two", "success"), one("exact_three", "success")) == (1, 1)
    assert (one("need_four", "success"), one("need_four", "n_corrections"), one("need_four", "num_conflicts_after")) == (0, 3, 1)
    assert one("need_four", "score") == 0.0
    assert one("restore", "corr_cells") == [[0, 5, 7], [0, 7, 5], [0, 5, 7]]
    assert one("zero_alternative", "corr_cells")[0] == [0, 5, 0] and one("zero_alternative", "digits")[0] == 0
    assert one("zero_alternative", "index")[0] == [0, 5, 3]
    # three 7s in a row take two corrections, the two least confident cells, each to its best alternative
    assert one("three_in_row", "corr_cells")[:2] == [[0, 7, 1], [3, 7, 3]] and one("three_in_row", "paths_explored") == 7
    assert [c[0] for c in one("exact_two", "corr_cells")[:2]] == [0, 37] and [c[0] for c in one("exact_three", "corr_cells")] == [0, 28, 56]
    # 18 candidates cut to 10 per path: 1 + 10 + 5 * 10 + 5 * 10 paths
    assert one("cut_at_ten", "paths_explored") == 111 and one("need_four", "paths_explored") == 101


@pytest.mark.parametrize("name", sorted(rr.VARIANTS))
def test_other_arguments(ctx, golden, name):
    """k = 1, 2, 4; beam widths 1 and 6; 0 and 1 corrections."""
    seed, n, k, beam, maxc = rr.VARIANTS[name]
    index, prob = rr.frames(seed, n, k)
    got = run(ctx, index, prob, beam_width=beam, max_corrections=maxc)
    same(got, rr.resolve(index, prob, beam, maxc), name)
    same(got, from_golden(golden, f"var.{name}"), f"{name} against the reference's results")


# ---- real probabilities ---------------------------------------------------------------------------------------------------------------
REAL_SETS = {"real": (rr.REAL_SEED, rr.REAL_N, 3), **rr.REAL_VARIANTS}
ALL_REAL = sorted(REAL_SETS) + [rr.minalt_name(m) for m in rr.MINALT]
_REAL = {}


def real_set(name):
    """-> (index, prob, min_alt, the restatement's results), computed once."""
    if name not in _REAL:
        if name in REAL_SETS:
            (index, prob), m = rr.real_frames(*REAL_SETS[name]), 0.1
        else:
            m = next(m for m in rr.MINALT if rr.minalt_name(m) == name)
            index, prob = rr.minalt_frames(m)[:2]
        _REAL[name] = (index, prob, m, rr.resolve(index, prob, min_alt=m))
    return _REAL[name]


@pytest.mark.parametrize("name", ALL_REAL)
def test_real_frames_one_batch(ctx, golden, name):
    """k = 3, 2 and 4 at the default threshold, and the thresholds that f32 rounds down (an alternative of exactly np.float32(m) is
    not eligible, one ulp above it is)."""
    index, prob, m, want = real_set(name)
    got = run(ctx, index, prob, min_alternative_confidence=m)
    same(got, want, f"{name}, one launch")
    same(got, from_golden(golden, name), f"{name} against the reference's results")


@pytest.mark.parametrize("batch", [1, 5])
def test_real_frames_small_batches(ctx, batch):
    index, prob, _, want = real_set("real")
    same(run(ctx, index, prob, batch=batch), want, f"real frames in launches of {batch}")


def test_real_frames_do_not_depend_on_the_batch(ctx):
    index, prob, _, want = real_set("real")
    rows = np.nonzero(want["num_conflicts_before"] > 0)[0]
    assert 0 < rows.size < index.shape[0]
    same(run(ctx, index[rows], prob[rows]), want, "real frames, valid frames removed", rows)


@pytest.mark.parametrize("name", ["real", rr.minalt_name(rr.MINALT[0])])
def test_real_frames_acceptance_rule(ctx, name):
    index, prob, m, want = real_set(name)
    expect, take = _accepted(want, index, prob)
    assert (~take).any() and (want["success"] != 0).any() and ((take & (want["success"] == 0)).any() or name != "real")
    same(run(ctx, index, prob, min_alternative_confidence=m, acceptance_rule=True), expect, f"{name}, acceptance rule")


def test_softmax_topk_feeds_resolve(ctx):
    """The chain as production runs it: k_softmax_topk on real logits, its own index and prob into K9 on the device and, copied to
    the host, into the restatement.  The GPU's expf may put an alternative on the other side of 0.1 than a CPU softmax would, so both
    sides take the GPU's top-3; what must hold first is the domain: top-1 of a filled cell >= 2^-18."""
    n = 64
    logits = torch.from_numpy(rr.real_logits(rr.REAL_SEED, n)).to(ctx.device)
    idx, prob = ctx.softmax_topk(logits.reshape(n * 81, 10), 3)
    idx, prob = idx.view(n, 81, 3), prob.view(n, 81, 3)
    hi, hp = idx.cpu().numpy(), prob.cpu().numpy()
    assert np.isfinite(hp).all() and (hp[:, :, 0][hi[:, :, 0] > 0] >= rr.DOMAIN_FLOOR).all()
    assert (hi == real_set("real")[0][:n]).mean() > 0.99                      # the same frames, up to near-ties
    want = rr.resolve(hi, hp)
    stats = want["stats"]
    assert (want["num_conflicts_before"] == 0).sum() >= 5 and (stats[:, 0] == 1).sum() >= 2 and (stats[:, 0] >= 2).sum() >= 5 and (want["success"] == 0).sum() >= 5
    got = ctx.resolve_conflicts(idx, prob)
    same({key: got[key].cpu().numpy() for key in rr.FIELDS}, want, "K9 on k_softmax_topk's output")


def test_argument_ranges(ctx):
    import sudoku_vision_amd as sva
    index, prob = rr.frames(1, 2)
    di, dp = torch.from_numpy(index).to(ctx.device), torch.from_numpy(prob).to(ctx.device)
    for kw in ({"beam_width": 0}, {"beam_width": 7}, {"max_corrections": -1}, {"max_corrections": 4}):
        with pytest.raises(sva._native.NativeError, match="SV_ERR_UNSUPPORTED"):
            ctx.resolve_conflicts(di, dp, **kw)
    with pytest.raises(sva._native.NativeError, match="SV_ERR_UNSUPPORTED"):          # k = 0
        ctx.resolve_conflicts(di[:, :, :0], dp[:, :, :0])
    i5, p5 = rr.frames(1, 2, 5)
    with pytest.raises(sva._native.NativeError, match="SV_ERR_UNSUPPORTED"):
        ctx.resolve_conflicts(torch.from_numpy(i5).to(ctx.device), torch.from_numpy(p5).to(ctx.device))
    empty = ctx.resolve_conflicts(di[:0], dp[:0])
    assert empty["digits"].shape == (0, 81) and empty["score"].shape == (0,)


# ---- the drop-in modules -------------------------------------------------------------------------------------------------------------
def _dropins():
    d = os.path.join(ROOT, "sudoku-vision_amd", "resolve")
    if d not in sys.path:
        sys.path.insert(0, d)
    import conflict_resolver
    import validator
    return validator, conflict_resolver


def _cells(validator, index, prob):
    return [validator.CellInfo(row=x // 9, col=x % 9, digit=int(index[x, 0]), confidence=float(prob[x, 0]),
                               alternatives=[(int(index[x, j]), float(prob[x, j])) for j in range(1, index.shape[1])]) for x in range(81)]


def _check_dropin(validator, resolver, index, prob, golden, prefix, f):
    cells = _cells(validator, index, prob)
    first = validator.validate_predictions(cells)
    res = resolver.resolve_conflicts(cells)
    g = {key: golden[f"{prefix}.{key}"][f] for key in rr.FIELDS + ("descriptions",)}
    before, after = str(g["descriptions"]).split("||")
    assert "|".join(c.description for c in first.conflicts) == before and first.num_conflicts == g["num_conflicts_before"]
    assert first.is_valid == (g["num_conflicts_before"] == 0) and first.num_cells_affected == len(first.cells_in_conflict)
    assert "|".join(c.description for c in res.validation_result.conflicts) == after
    assert (res.success, res.paths_explored, res.validation_result.num_conflicts) == (bool(g["success"]), g["paths_explored"], g["num_conflicts_after"])
    assert np.float64(res.score).tobytes() == g["score"].tobytes()
    assert res.grid == g["digits"].reshape(9, 9).tolist()
    assert [(9 * m.row + m.col, m.original_digit, m.new_digit) for m in res.corrections_made] == [tuple(v) for v in g["corr_cells"][:g["n_corrections"]].tolist()]
    assert [(np.float32(m.original_confidence), np.float32(m.alternative_confidence)) for m in res.corrections_made] == \
           [tuple(v) for v in g["corr_conf"][:g["n_corrections"]]]
    for c in res.cells:
        x = 9 * c.row + c.col
        keep = g["index"][x, 1:] != rr.PAD_INDEX
        assert (c.digit, np.float32(c.confidence)) == (g["index"][x, 0], g["prob"][x, 0])
        assert [d for d, _ in c.alternatives] == g["index"][x, 1:][keep].tolist()
        assert [np.float32(p) for _, p in c.alternatives] == g["prob"][x, 1:][keep].tolist()


def test_dropin_modules_on_the_selftest_and_generated_frames(ctx, golden, generated):
    validator, resolver = _dropins()
    index, prob = rr.crafted_cases()["selftest"]
    _check_dropin(validator, resolver, index[0], prob[0], golden, "case.selftest", 0)
    for f in range(8):
        _check_dropin(validator, resolver, generated[0][f], generated[1][f], golden, "gen", f)


def test_dropin_selftest_cells_as_the_reference_writes_them(ctx):
    """conflict_resolver.py:293-322 as written: python floats and cells without alternatives."""
    validator, resolver = _dropins()
    cells = [validator.CellInfo(row=i // 9, col=i % 9, digit=0, confidence=0.9) for i in range(81)]
    cells[0] = validator.CellInfo(row=0, col=0, digit=5, confidence=0.95, alternatives=[(3, 0.03), (6, 0.02)])
    cells[1] = validator.CellInfo(row=0, col=1, digit=3, confidence=0.88, alternatives=[(8, 0.05), (2, 0.04)])
    cells[3] = validator.CellInfo(row=0, col=3, digit=5, confidence=0.6, alternatives=[(8, 0.25), (9, 0.10)])
    first = validator.validate_predictions(cells)
    assert [c.description for c in first.conflicts] == ["Row 1: digit 5 appears at columns [1, 4]"] and first.cells_in_conflict == {(0, 0), (0, 3)}
    res = resolver.resolve_conflicts(cells)
    assert res.success and res.paths_explored == 2 and res.grid[0][:4] == [5, 3, 0, 8] and res.validation_result.is_valid
    assert [(m.row, m.col, m.original_digit, m.new_digit) for m in res.corrections_made] == [(0, 3, 5, 8)]
    assert res.cells[3].alternatives == [(5, float(np.float32(0.6))), (9, float(np.float32(0.10)))] and res.cells[4].alternatives == []
    with pytest.raises(ValueError):
        validator.validate_predictions([validator.CellInfo(row=i // 9, col=i % 9, digit=0, alternatives=[(1, 0.1)] * 4) for i in range(81)])


# ---- the acceptance rule and out= -----------------------------------------------------------------------------------------------------
def _accepted(want, index, prob):
    """run_v2's acceptance rule (pipeline/run_v2.py:365) on the restatement's results: a repair that neither succeeded nor left fewer
    conflicts is dropped, and the cell outputs, the conflicts after and the corrections are the input's."""
    take = (want["success"] != 0) | (want["num_conflicts_after"] < want["num_conflicts_before"])
    plain = rr.resolve(index, prob, max_corrections=0)          # no correction allowed: the input, validated
    out = {}
    for key in rr.FIELDS:
        t = take.reshape((-1,) + (1,) * (want[key].ndim - 1))
        out[key] = np.where(t, want[key], plain[key]) if key not in ("success", "paths_explored", "score") else want[key]
    return out, take


def test_acceptance_rule_in_the_kernel(ctx, generated):
    index, prob, want = generated
    expect, take = _accepted(want, index, prob)
    assert 25 < (~take).sum() and 25 < (take & (want["success"] == 0)).sum() and 25 < (want["success"] != 0).sum()
    same(run(ctx, index, prob, acceptance_rule=True), expect, "acceptance rule")


def test_out_tensors_are_written_in_place(ctx, generated):
    index, prob, want = generated
    di, dp = torch.from_numpy(index[:40]).to(ctx.device), torch.from_numpy(prob[:40]).to(ctx.device)
    digits = torch.full((48, 81), 77, dtype=torch.uint8, device=ctx.device)
    ncorr = torch.full((40,), 77, dtype=torch.uint8, device=ctx.device)
    got = ctx.resolve_conflicts(di, dp, out={"digits": digits[4:44], "n_corrections": ncorr})
    assert set(got) == {"digits", "n_corrections"} and got["n_corrections"] is ncorr
    assert (digits[4:44].cpu().numpy() == want["digits"][:40]).all() and (digits[:4] == 77).all() and (digits[44:] == 77).all()
    assert (ncorr.cpu().numpy() == want["n_corrections"][:40]).all()
    with pytest.raises(TypeError):
        ctx.resolve_conflicts(di, dp, out={"digits": digits})
    with pytest.raises(KeyError):
        ctx.resolve_conflicts(di, dp, out={"grid": digits})


# ---- the pipeline: recognised logits are replaced by chosen ones where the CNN hands them over ------------------------------------------
def _puzzle(seed):
    """-> (shown [81]: a solved grid with 45 cells blank, truth [81])"""
    truth = rr._solved(np.random.RandomState(seed))
    shown = truth.copy()
    shown[np.random.RandomState(seed + 1000).permutation(81)[:45]] = 0
    return shown, truth


def _misread(shown, truth, count, seed):
    """`count` shown cells in different rows, columns and boxes, each with the digit of a shown peer -> {cell: wrong digit}"""
    rs, out = np.random.RandomState(seed), {}
    for x in rs.permutation(81):
        x = int(x)
        clear = all(x // 9 != y // 9 and x % 9 != y % 9 and rr.BOXES.index(next(b for b in rr.BOXES if x in b)) !=
                    rr.BOXES.index(next(b for b in rr.BOXES if y in b)) for y in out)
        peers = [y for y in rr._peers(x) if shown[y] > 0 and shown[y] != shown[x] and y not in out]
        if shown[x] > 0 and clear and peers and len(out) < count:
            out[x] = int(shown[peers[0]])
    assert len(out) == count
    return out


def _logits(shown, truth, wrong, runner_up=True):
    """Logits [81,10] of a sure recogniser (top-1 0.9996) that misreads the cells of `wrong`; with runner_up the misread is unsure
    (0.62) and the true digit is its second choice (0.38), without it the misread is as sure as the rest: no alternative reaches 0.1."""
    logits = np.full((81, 10), -4.0, np.float32)
    logits[np.arange(81), shown] = 6.0
    for x, d in wrong.items():
        logits[x] = -4.0
        logits[x, d] = 3.0 if runner_up else 6.0
        if runner_up:
            logits[x, truth[x]] = 2.5
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


def test_stage_corrects_a_cell_whose_runner_up_is_the_truth(ctx):
    from sudoku_vision_amd.pipeline import _validate_and_resolve
    shown, truth = _puzzle(5)
    (x, d), = _misread(shown, truth, 1, 6).items()
    logits = _logits(shown, truth, {x: d})
    res = _validate_and_resolve(ctx, *[t[None] for t in ctx.softmax_topk(torch.from_numpy(logits).to(ctx.device), 3)])
    assert res["resolved_grid"] == shown.reshape(9, 9).tolist() and res["validation"] == {"is_valid": True, "num_conflicts": 0, "cells_in_conflict": []}
    assert [c[:4] for c in res["corrections"]] == [(x // 9, x % 9, d, int(truth[x]))] and res["paths_explored"] == 2


def test_recognize_image_resolve(ctx, golden_dir, monkeypatch):
    from sudoku_vision_amd import imgcodecs
    from sudoku_vision_amd.pipeline import recognize_image
    from sudoku_vision_amd.synth import random_state_dict
    sd = random_state_dict(99)
    img = imgcodecs.imread(os.path.join(golden_dir, "sample_1.jpg"))
    plain = recognize_image(img, sd, ctx=ctx)
    shown, truth = _puzzle(11)
    (x, d), = _misread(shown, truth, 1, 12).items()
    read = shown.copy()
    read[x] = d
    # the misread cell's runner-up is the truth: one correction, taken
    _inject(monkeypatch, ctx, torch.from_numpy(_logits(shown, truth, {x: d})).to(ctx.device)[None])
    base = recognize_image(img, sd, ctx=ctx)
    res = recognize_image(img, sd, ctx=ctx, resolve=True)
    assert set(base) == set(plain) and set(res) - set(base) == {"alternatives", "validation", "corrections", "resolved_grid", "paths_explored"}
    for key in base:
        assert np.array_equal(np.asarray(res[key]), np.asarray(base[key])), key
    assert res["grid"] == read.reshape(9, 9).tolist() and res["resolved_grid"] == shown.reshape(9, 9).tolist()
    assert res["validation"] == {"is_valid": True, "num_conflicts": 0, "cells_in_conflict": []} and res["paths_explored"] == 2
    (r, c, old, new, c_old, c_new), = res["corrections"]
    assert (r, c, old, new) == (x // 9, x % 9, d, int(truth[x])) and res["alternatives"][x][0] == (int(truth[x]), c_new)
    assert abs(c_old - 0.62) < 0.01 and abs(c_new - 0.376) < 0.01
    # no alternative reaches 0.1: nothing to try, the repair is not taken and the validation is the input's
    _inject(monkeypatch, ctx, torch.from_numpy(_logits(shown, truth, {x: d}, runner_up=False)).to(ctx.device)[None])
    res = recognize_image(img, sd, ctx=ctx, resolve=True)
    assert res["resolved_grid"] == res["grid"] == read.reshape(9, 9).tolist() and res["corrections"] == [] and res["paths_explored"] == 1
    assert not res["validation"]["is_valid"] and res["validation"]["num_conflicts"] >= 1 and (x // 9, x % 9) in res["validation"]["cells_in_conflict"]


def test_frame_pipeline_resolve(ctx, monkeypatch):
    """Frame f of the pool is read as: f % 4 == 0 a valid grid; 1 one misread cell whose runner-up is the truth (repaired); 2 one
    misread cell without an alternative (nothing to try: not taken); 3 four misread cells with the truth as runner-up (three
    corrections leave one conflict: taken, not a success).  Frame 5 is blank: no grid."""
    from sudoku_vision_amd.pipeline import FramePipeline
    from sudoku_vision_amd.synth import synth_frames, random_state_dict
    ctx.load_state_dict(random_state_dict(1234))
    n, H, W = 24, 270, 480
    frames, _, _ = synth_frames(n, H, W, seed=17, device="cuda")
    frames = frames.contiguous()
    frames[5] = 0
    plain = FramePipeline(ctx, H, W, chunk=8, depth=3)
    before = plain.run(frames)
    shown_all, read_all, logits = [], [], []
    for f in range(n):
        shown, truth = _puzzle(100 + f)
        wrong = _misread(shown, truth, (0, 1, 1, 4)[f % 4], 200 + f)
        read = shown.copy()
        for x, d in wrong.items():
            read[x] = d
        shown_all.append(shown)
        read_all.append(read)
        logits.append(_logits(shown, truth, wrong, runner_up=f % 4 != 2))
    shown_all, read_all = np.stack(shown_all), np.stack(read_all)
    crafted = torch.from_numpy(np.stack(logits)).to(ctx.device)
    torch.cuda.synchronize()
    _inject(monkeypatch, ctx, crafted, frames)
    off = plain.run(frames)
    p = FramePipeline(ctx, H, W, chunk=8, depth=3, resolve=True)
    on = p.run(frames)
    assert set(off) == set(before) == {"logits", "digits", "conf", "corners", "found"}
    assert set(on) - set(off) == {"resolved_digits", "resolve_success", "num_conflicts", "n_corrections"}
    for key in ("digits", "logits", "conf"):
        assert torch.equal(off[key], on[key]), key
    assert (off["corners"] == on["corners"]).all() and (off["found"] == on["found"]).all()
    assert plain.describe() != p.describe() and plain.describe() == FramePipeline(ctx, H, W, chunk=8, depth=3, resolve=False).describe()
    found = on["found"]
    assert not found[5] and found.sum() == n - 1
    kind = np.arange(n) % 4
    got = {key: on[key].cpu().numpy() for key in ("digits", "resolved_digits", "resolve_success", "num_conflicts", "n_corrections")}
    assert on["resolve_success"].dtype == torch.bool
    assert (got["digits"][found] == read_all[found]).all()
    for f in np.nonzero(found)[0]:
        what = f"frame {f} kind {kind[f]}"
        if kind[f] in (0, 1):
            assert (got["resolved_digits"][f] == shown_all[f]).all() and got["resolve_success"][f] and got["num_conflicts"][f] == 0, what
            assert got["n_corrections"][f] == kind[f], what
        elif kind[f] == 2:
            assert (got["resolved_digits"][f] == read_all[f]).all() and not got["resolve_success"][f], what
            assert got["num_conflicts"][f] >= 1 and got["n_corrections"][f] == 0, what
        else:
            assert got["n_corrections"][f] == 3 and not got["resolve_success"][f] and got["num_conflicts"][f] >= 1, what
            assert (got["resolved_digits"][f] != read_all[f]).sum() == 3 and (got["resolved_digits"][f] != shown_all[f]).sum() == 1, what
    assert not got["resolved_digits"][5].any() and not got["resolve_success"][5] and got["num_conflicts"][5] == 0 and got["n_corrections"][5] == 0
    # and all of it against the restatement on the same top-3
    idx, prob = ctx.softmax_topk(crafted.reshape(-1, 10), 3)
    idx, prob = idx.view(n, 81, 3).cpu().numpy(), prob.view(n, 81, 3).cpu().numpy()
    expect, _ = _accepted(rr.resolve(idx, prob), idx, prob)
    for key, name in (("resolved_digits", "digits"), ("resolve_success", "success"), ("num_conflicts", "num_conflicts_after"), ("n_corrections", "n_corrections")):
        assert (got[key][found] == expect[name][found]).all(), key


def test_frame_pipeline_resolve_real_logits(ctx, monkeypatch):
    """FramePipeline(resolve=True) with the generator's real logits handed over in place of the CNN's: full-mantissa confidences
    through softmax_topk, K9 and the acceptance rule, against the restatement on the GPU's own top-3."""
    from sudoku_vision_amd.pipeline import FramePipeline
    from sudoku_vision_amd.synth import synth_frames, random_state_dict
    ctx.load_state_dict(random_state_dict(1234))
    n, H, W = 24, 270, 480
    frames, _, _ = synth_frames(n, H, W, seed=17, device="cuda")
    frames = frames.contiguous()
    crafted = torch.from_numpy(rr.real_logits(rr.REAL_SEED + 5, n)).to(ctx.device)
    torch.cuda.synchronize()
    _inject(monkeypatch, ctx, crafted, frames)
    on = FramePipeline(ctx, H, W, chunk=8, depth=3, resolve=True).run(frames)
    found = on["found"]
    assert found.sum() >= n - 1
    got = {key: on[key].cpu().numpy() for key in ("digits", "resolved_digits", "resolve_success", "num_conflicts", "n_corrections")}
    idx, prob = ctx.softmax_topk(crafted.reshape(-1, 10), 3)
    idx, prob = idx.view(n, 81, 3).cpu().numpy(), prob.view(n, 81, 3).cpu().numpy()
    assert (prob[:, :, 0][idx[:, :, 0] > 0] >= rr.DOMAIN_FLOOR).all() and (got["digits"][found] == idx[:, :, 0][found]).all()
    want = rr.resolve(idx, prob)
    expect, take = _accepted(want, idx, prob)
    assert (want["num_conflicts_before"] == 0).any() and (want["n_corrections"][take] > 0).any() and (~take).any() and (take & (want["success"] == 0)).any()
    for key, name in (("resolved_digits", "digits"), ("resolve_success", "success"), ("num_conflicts", "num_conflicts_after"), ("n_corrections", "n_corrections")):
        assert (got[key][found] == expect[name][found]).all(), key
