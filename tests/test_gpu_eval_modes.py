"""GPU (-m gpu): K21 (csrc/k21_eval.hip) through Context.eval_metrics where tests/test_gpu_eval.py does not go, against tests/eval_ref.py.

1 probability mode   every per-cell output, the aggregates for every edge set and the failure records on eval_ref.prob_cells(): softmax
                     rows with denormal and zero entries, and crafted rows (confidences of 0 and below 2^-30, negative entries, the
                     mode's own finite rule, NaN / Inf, maxima exactly on f32(0.1), f32(0.3), f32(0.7), 0.125)
2 caller bin edges   logits mode with every entry of eval_ref.EDGE_SETS: non-uniform, repeated, not spanning [0, 1], edges f32 cannot
                     represent, 65 edges of the caller's own; the crafted 1.0 / 0.5 / 0.25 cells by hand; edges the entry refuses
3 long failure list  262,146 cells with 300 wrong ones placed on the seams of k_eval_scan's 256-tile chunks and of a workgroup's second
                     tile; lists that end at each of them; the unwritten tail
4 long, accumulated  the same cells in three accumulating calls split off the tile boundary, with the list already full, and with a
                     middle call that asks for no list
5 drop-in at size    evaluate_v2.compute_calibration on 4,097 rows against the reference's lines

Every reference value comes from the restatement (per_cell_prob, aggregates, aggregates_fast, calibration), none from the kernel, but for
test 2's aggregates, which -- as in tests/test_gpu_eval.py -- bin the kernel's own f32 conf."""
import os
import sys

import numpy as np
import pytest
import torch

import cnn_oracle
import eval_ref as er
import test_gpu_softmax_topk as tk

pytestmark = pytest.mark.gpu
ALL = ("probs", "pred", "conf", "true_prob", "nll", "correct")
FILL = 0xA5                                    # what a failure buffer holds before the call: an unwritten record keeps it


def dev(ctx, a):
    return torch.from_numpy(np.array(a)).to(ctx.device)                      # a copy: the shared inputs are not writable


def run(ctx, z, labels, **kw):
    out, agg = ctx.eval_metrics(dev(ctx, z), dev(ctx, labels), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, agg


def bad_arg():
    import sudoku_vision_amd as sva
    return pytest.raises(sva._native.NativeError, match="SV_ERR_BAD_ARG")


# ---- 1: probability mode ---------------------------------------------------------------------------------------------------------------------
def test_probability_mode(ctx):
    """Test 1.  probs, conf and true_prob are the input's bytes; pred is np.argmax on every row (the NaN row included); correct is
    pred == label on the rows the mode's finite rule keeps and 0 elsewhere (include/sudoku_vision_hip.h); nll is exact where it is
    infinite or NaN and within cnn_oracle.tolerance of the float64 -log elsewhere, the noise being numpy's own f32 -log against float64
    on the same rows; the aggregates are the restatement's for every edge set with the restatement's finite flag; the failure records
    are the wrong valid cells in order with the input's bytes and a stable descending top-3."""
    probs, labels, marks = er.prob_cells()
    r = er.per_cell_prob(probs, labels)
    rows = np.arange(len(probs))
    wrong = np.nonzero(r["finite"] & ~r["correct"])[0]
    out, agg = run(ctx, probs, labels, probabilities=True, want=ALL, max_failures=len(wrong) + 5)
    assert out["probs"].tobytes() == probs.tobytes()
    assert (out["pred"] == r["pred"]).all(), np.nonzero(out["pred"] != r["pred"])[0]
    assert out["conf"].tobytes() == probs[rows, r["pred"]].tobytes() == r["conf"].tobytes()
    assert out["true_prob"].tobytes() == probs[rows, labels].tobytes() == r["true_prob"].tobytes()
    assert (out["correct"].astype(bool) == (r["correct"] & r["finite"])).all()
    # nll
    fin = np.isfinite(r["nll"])
    assert fin.sum() > 400 and np.isposinf(r["nll"]).sum() > 0 and np.isnan(r["nll"]).sum() >= 2
    assert np.array_equal(out["nll"][~fin].astype(np.float64), r["nll"][~fin], equal_nan=True), "+inf, -inf and NaN where the float64 -log has them"
    assert out["nll"][marks["zeros"]] == np.inf and np.isnan(out["nll"][[marks["negatives"], marks["neg_label"]]]).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        numpy32 = (-np.log(r["true_prob"])).astype(np.float64)
    assert numpy32.dtype == np.float64 and r["true_prob"].dtype == np.float32
    noise = np.abs(numpy32[fin] - r["nll"][fin]).max()
    tol = cnn_oracle.tolerance(r["nll"][fin], noise, tk.C_ABS)
    err = np.abs(out["nll"][fin].astype(np.float64) - r["nll"][fin]).max()
    print(f"probability mode: max|nll - f64| {err:.3e}, noise {noise:.3e}, bound {tol:.3e} (largest finite nll {r['nll'][fin].max():.2f})")
    assert np.isfinite(out["nll"][fin]).all() and err <= tol
    # aggregates, every edge set
    pd, ld = dev(ctx, probs), dev(ctx, labels)
    for name, (edges, n_bins) in er.EDGE_SETS.items():
        _, got = ctx.eval_metrics(pd, ld, n_bins=n_bins, bin_edges=edges, probabilities=True, want=())
        assert got == er.aggregates(r["pred"], r["conf"], labels, n_bins, finite=r["finite"], edges=edges), name
    assert agg == er.aggregates(r["pred"], r["conf"], labels, 10, finite=r["finite"]) and agg["nonfinite"] == 4 and agg["n_wrong"] == len(wrong)
    # failure records
    rec = ctx.eval_failures(torch.from_numpy(out["failures"]), len(wrong))
    assert rec["index"].tolist() == wrong.tolist() and {marks[k] for k in ("negatives", "neg_label")} <= set(wrong.tolist())
    assert rec["label"].tolist() == labels[wrong].tolist() and rec["pred"].tolist() == r["pred"][wrong].tolist()
    assert rec["conf"].tobytes() == r["conf"][wrong].tobytes() and rec["true_prob"].tobytes() == r["true_prob"][wrong].tobytes()
    for f in rec:
        p = probs[f["index"]]
        order = np.argsort(-p, kind="stable")[:3]                          # stable: equal entries lowest class first
        assert f["top3_index"].tolist() == order.tolist() and f["top3_prob"].tobytes() == p[order].tobytes(), int(f["index"])
    neg = rec[wrong.tolist().index(marks["negatives"])]
    assert neg["top3_index"].tolist() == [4, 1, 5] and neg["top3_prob"].tolist() == [np.float32(0.6), -1.0, -1.0]
    with bad_arg():
        ctx.eval_metrics(pd, ld, probabilities=True, temperature=2.0)


# ---- 2: logits mode with the caller's edges -------------------------------------------------------------------------------------------------
BY_HAND = {     # bin_count, bin_correct, bin_conf / 2^28 of crafted_cells(): see test_logits_mode_with_caller_edges
    "decimal": ([0, 4, 4, 8], [0, 1, 1, 6], [0, 4, 8, 32]),
    "repeated": ([8, 0, 0, 8], [2, 0, 0, 6], [12, 0, 0, 32]),
    "inner": ([4, 4], [1, 1], [4, 8]),
    "one": ([16], [8], [44]),
}


@pytest.mark.parametrize("name", list(er.EDGE_SETS))
def test_logits_mode_with_caller_edges(ctx, name):
    """Test 2.  257 cells at each scale and crafted_cells() in one call: the aggregates are the restatement's on the kernel's pred and conf.
    Then crafted_cells() alone, by hand: 8 cells of conf 1.0 (6 correct), 4 of 0.5 (1 correct), 4 of 0.25 (1 correct), a cell being in
    bin i when edges[i] < conf <= edges[i + 1]:
      decimal  [0, .1, .3, .7, 1]   0.25 in (.1, .3] = bin 1, 0.5 in (.3, .7] = bin 2, 1.0 on the closed top edge of bin 3
      repeated [0, .5, .5, .5, 1]   0.25 and 0.5 both in (0, .5] = bin 0 (8 cells, 2 correct, 4 * .25 + 4 * .5 = 3); bins 1 and 2 are
                                    (.5, .5]: empty; 1.0 in bin 3
      inner    [.2, .4, .9]         0.25 in bin 0, 0.5 in bin 1, 1.0 above the last edge: in no bin, yet in n and the totals
      one      [.125, 1]            all 16 in the one bin: 8 correct, 8 * 1 + 4 * .5 + 4 * .25 = 11"""
    edges, n_bins = er.EDGE_SETS[name]
    cz, cl, _, _ = er.crafted_cells()
    parts = [(er.random_cells(s)[0][:257], er.random_cells(s)[1][:257]) for s in er.SCALES] + [(cz, cl)]
    z, labels = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    out, agg = run(ctx, z, labels, n_bins=n_bins, bin_edges=edges, want=("pred", "conf"))
    assert agg == er.aggregates(out["pred"], out["conf"], labels, n_bins, edges=edges) and agg["n"] == 530
    out, agg = run(ctx, cz, cl, n_bins=n_bins, bin_edges=edges, want=("pred", "conf"))
    assert out["conf"].tolist() == [1.0] * 8 + [0.5] * 4 + [0.25] * 4
    assert agg == er.aggregates(out["pred"], out["conf"], cl, n_bins, edges=edges)
    assert (agg["n"], agg["n_correct"]) == (16, 8) and agg["tot_count"] == [16, 8, 8] and agg["tot_conf"][0] == 11 << 30
    if name in BY_HAND:
        count, good, quarters = BY_HAND[name]
        assert (agg["bin_count"], agg["bin_correct"], agg["bin_conf"]) == (count, good, [q << 28 for q in quarters])


def test_edges_the_entry_refuses(ctx):
    z, labels = er.random_cells(1.0)
    zd, ld = dev(ctx, z[:65]), dev(ctx, labels[:65])
    with bad_arg():
        ctx.eval_metrics(zd, ld, n_bins=4, bin_edges=[0, 0.5, 0.25, 0.75, 1.0])
    with bad_arg():
        ctx.eval_metrics(zd, ld, n_bins=4, bin_edges=[0, 0.25, float("nan"), 0.75, 1.0])
    with pytest.raises(ValueError, match="n_bins"):
        ctx.eval_metrics(zd, ld, n_bins=4, bin_edges=[0, 0.25, 0.5, 1.0])
    with pytest.raises(ValueError, match="n_bins"):
        ctx.eval_metrics(zd, ld, n_bins=4, bin_edges=np.linspace(0, 1, 6))


# ---- 3 and 4: the long failure list ----------------------------------------------------------------------------------------------------------
SPLITS = (0, 65600, 200000, er.SIZES[-1])      # 65,600 = 256 * 256 + 64: past the scan seam and on no tile boundary


def long_limits(wrong):
    """max_failures by where the list then ends."""
    seam = int(np.searchsorted(wrong, 65536))                               # the wrong cells below 65,536
    return {"inside tile 0": 1, "one short of the seam": seam - 1, "at the seam": seam, "one past the seam": seam + 1,
            "inside the all-wrong tile": int(np.searchsorted(wrong, er.LONG_TILE * 256)) + 100, "on cell 262,144": int(np.searchsorted(wrong, 262144)) + 1,
            "beyond n_wrong": len(wrong) + 7}


@pytest.fixture(scope="module")
def long(ctx):
    """The long list's cells on the device, and the aggregates the vectorised twin gives for the kernel's pred and conf of one call."""
    z, labels, wrong = er.long_list_cells()
    zd, ld = dev(ctx, z), dev(ctx, labels)
    out, agg = ctx.eval_metrics(zd, ld, want=("pred", "conf"))
    pred = out["pred"].cpu().numpy()
    assert (pred == z.argmax(1)).all()
    want = er.aggregates_fast(pred, out["conf"].cpu().numpy(), labels, 10)
    assert agg == want and want["n_wrong"] == len(wrong) == 300
    return {"z": z, "labels": labels, "wrong": wrong, "pred": pred, "zd": zd, "ld": ld, "agg": want, "stats": out["stats"].cpu().numpy().tobytes()}


def filled(ctx, n):
    return torch.full((n, 48), FILL, dtype=torch.uint8, device=ctx.device)


def check_records(ctx, buf, long, places, cells):
    """Records `places` of the buffer are the wrong cells `cells`, every other record of the buffer is untouched."""
    raw = buf.cpu().numpy()
    rec = ctx.eval_failures(buf, len(raw))
    places = np.asarray(places, np.int64)
    assert rec["index"][places].tolist() == cells.tolist()
    assert rec["label"][places].tolist() == long["labels"][cells].tolist() and rec["pred"][places].tolist() == long["pred"][cells].tolist()
    assert (rec["top3_index"][places, 0] == long["pred"][cells]).all()
    rest = np.ones(len(raw), bool)
    rest[places] = False
    assert (raw[rest] == FILL).all(), "a record outside the list was written"
    assert not (raw[~rest] == FILL).all(1).any()


@pytest.mark.parametrize("where", list(long_limits(er.LONG_SEAMS)))
def test_long_failure_list(ctx, long, where):
    """Test 3: one call over 262,146 cells (1,025 tiles: five chunks of k_eval_scan, a second tile for workgroup 0)."""
    wrong = long["wrong"]
    m = long_limits(wrong)[where]
    n = min(m, len(wrong))
    last, following = int(wrong[n - 1]), int(wrong[n]) if n < len(wrong) else None       # the list's last cell, the first one left out
    assert 0 < m and {"inside tile 0": last < 256, "one short of the seam": following == 65535, "at the seam": (last, following) == (65535, 65536),
                      "one past the seam": last == 65536, "inside the all-wrong tile": following is not None and last // 256 == er.LONG_TILE == following // 256,
                      "on cell 262,144": last == 262144, "beyond n_wrong": m > n == 300}[where]
    buf = filled(ctx, m)
    out, agg = ctx.eval_metrics(long["zd"], long["ld"], max_failures=m, failures=buf, want=())
    assert agg == long["agg"] and agg["n_wrong"] == 300
    check_records(ctx, buf, long, np.arange(n), wrong[:n])


def accumulated(ctx, long, limits, buf):
    """The three parts of SPLITS as accumulating calls with max_failures limits[k] -> the stats block's bytes."""
    stats = ctx.eval_stats_buffer()
    for (a, b), m in zip(zip(SPLITS[:-1], SPLITS[1:]), limits):
        ctx.eval_metrics(long["zd"][a:b], long["ld"][a:b], max_failures=m, failures=buf if m else None, stats=stats, accumulate=True, index_base=a, want=(),
                         read_back=False)
    torch.cuda.synchronize()
    return stats.cpu().numpy().tobytes()


def test_long_failure_list_accumulated(ctx, long):
    """Test 4.  One call and three accumulating calls leave the same bytes, with a list that takes every wrong cell, one that is full
    after the first call (the second and third start on a full list) and one that fills inside the second.  Then the middle call asks
    for no list: by the header of sv_eval_metrics its wrong cells still take their places -- a record's place counts the wrong cells
    since the last clear of stats, whatever max_failures each call had -- so the third call's records start behind them and the
    places of the middle call's wrong cells stay unwritten."""
    wrong = long["wrong"]
    a, ab = (int(np.searchsorted(wrong, s)) for s in SPLITS[1:3])
    assert 2 < a < ab - 3 and ab + 3 < 300, "every part has wrong cells"
    for m in (307, a - 2, a + 3):
        one = filled(ctx, m)
        ctx.eval_metrics(long["zd"], long["ld"], max_failures=m, failures=one, want=(), read_back=False)
        parts = filled(ctx, m)
        stats = accumulated(ctx, long, (m, m, m), parts)
        assert stats == long["stats"], m
        assert parts.cpu().numpy().tobytes() == one.cpu().numpy().tobytes(), m
    for m in (307, ab + 2):
        buf = filled(ctx, m)
        stats = accumulated(ctx, long, (m, 0, m), buf)
        assert stats == long["stats"], "n_wrong and every other count are the totals whatever max_failures is"
        n = min(m, 300)
        places = np.concatenate([np.arange(a), np.arange(ab, n)])
        check_records(ctx, buf, long, places, wrong[places])
        one = filled(ctx, m)
        ctx.eval_metrics(long["zd"], long["ld"], max_failures=m, failures=one, want=(), read_back=False)
        assert buf.cpu().numpy()[places].tobytes() == one.cpu().numpy()[places].tobytes()


# ---- 5: the drop-in at size ---------------------------------------------------------------------------------------------------------------------
def test_compute_calibration_at_size(ctx):
    """Test 5: evaluate_v2.compute_calibration on the f32 softmax of 4,097 cells against the reference's lines (eval_ref.calibration).
    The reference bins whatever dtype it is given and the drop-in converts to f32, so both are fed f32: they see the same values.
    Counts, centres and accuracies (ratios of equal integers in float64) are exact.  bin_confidences and ece: the reference (an f32
    mean) and the drop-in are each compared with the float64 mean of the same f32 confidences; the drop-in's error is bounded by
    cnn_oracle.tolerance on the reference's own error."""
    import sudoku_vision_amd as sva
    ml = os.path.join(os.path.dirname(sva.__file__), "ml")
    sys.path.insert(0, ml)
    try:
        sys.modules.pop("evaluate_v2", None)
        import evaluate_v2 as ev
    finally:
        sys.path.remove(ml)
    z, labels = er.random_cells(1.0)
    labels = labels[:4097].copy()                                           # the drop-in makes a tensor of it: writable
    probs = torch.softmax(torch.from_numpy(z[:4097].copy()), 1).numpy()
    assert probs.dtype == np.float32
    top, ok = probs.max(1), probs.argmax(1) == labels
    for n_bins in (10, 15):
        got = ev.compute_calibration(probs, labels, n_bins, device=ctx.device)
        want = er.calibration(top, ok, n_bins)
        assert got["bin_counts"] == want["bin_counts"] and sum(got["bin_counts"]) == 4097 and len(got["bin_counts"]) >= 5
        assert got["bin_centers"] == want["bin_centers"] and got["bin_accuracies"] == want["bin_accuracies"]
        edges = np.linspace(0, 1, n_bins + 1)
        mean64, acc = [], []
        for i in range(n_bins):
            m = (top > edges[i]) & (top <= edges[i + 1])
            if m.sum():
                mean64.append(top[m].astype(np.float64).mean())
                acc.append(ok[m].mean())
        mean64 = np.array(mean64)
        ref_err = np.abs(np.array(want["bin_confidences"], np.float64) - mean64).max()
        err = np.abs(np.array(got["bin_confidences"], np.float64) - mean64).max()
        tol = cnn_oracle.tolerance(mean64, ref_err, tk.C_ABS)
        print(f"compute_calibration n_bins {n_bins}: bin_confidences error {err:.3e}, the reference's {ref_err:.3e}, bound {tol:.3e}")
        assert err <= tol
        ece64 = float((np.abs(np.array(acc) - mean64) * np.array(want["bin_counts"]) / 4097).sum())
        ref_err, err = abs(want["ece"] - ece64), abs(got["ece"] - ece64)
        tol = cnn_oracle.tolerance(ece64, ref_err, tk.C_ABS)
        print(f"compute_calibration n_bins {n_bins}: ece {got['ece']!r}, float64 {ece64!r}, error {err:.3e}, the reference's {ref_err:.3e}, bound {tol:.3e}")
        assert err <= tol
