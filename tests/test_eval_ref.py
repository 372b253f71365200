"""CPU: the K21 yardstick (tests/eval_ref.py) against the reference's own results, and every input of tests/test_gpu_eval.py against what
it was built for -- a weak input fails here and not silently on the GPU.

The restatement is pinned twice: to tests/golden/eval_goldens.npz (what the reference's ml/evaluate_v2.py returned for a tiny model and
loader, tests/golden/make_eval_goldens.py) and, where a reference tree is at hand (SV_REFERENCE_ROOT, default the golden script's), to the
imported compute_calibration and evaluate_dataset themselves under torch CPU.  The latter skip where there is no such tree."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import eval_ref as er
import test_gpu_softmax_topk as tk

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_eval_goldens as mk  # noqa: E402
sys.path.pop(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "eval_goldens.npz"))


def close_tree(got, want, rel=1e-6):
    """Same keys, same kinds; floats within rel (the reference sums f32 confidences in f32, the restatement's callers may not)."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and [str(k) for k in got] == [str(k) for k in want], (list(got), list(want))
        for (_, g), (_, w) in zip(got.items(), want.items()):
            close_tree(g, w, rel)
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            close_tree(g, w, rel)
    elif isinstance(want, (float, np.floating)):
        assert got == pytest.approx(want, rel=rel, abs=1e-7), (got, want)
    else:
        assert got == want, (got, want)


def test_module_of_the_dropin_exists():
    """The one CPU test that fails without the feature's Python side: the drop-in file and the ctypes rows are there."""
    import sudoku_vision_amd as sva
    assert os.path.exists(os.path.join(os.path.dirname(sva.__file__), "ml", "evaluate_v2.py"))
    assert {"sv_eval_metrics", "sv_eval_metrics_host"} <= set(sva._native.SIGNATURES)
    import ctypes
    assert ctypes.sizeof(sva._native.EvalStats) == 8 * (100 + 5 + 3 * 64 + 9) and sva._native.EVAL_FAILURE_DTYPE.itemsize == 48


def test_restatement_matches_the_reference_results(golden):
    probs, preds, labels = golden["probabilities"], golden["predictions"], golden["labels"]
    want = json.loads(str(golden["dataset"]))
    got = er.dataset_metrics(probs, preds, labels, "golden")
    assert set(got) == set(want) | {"predictions", "labels", "probabilities"}
    close_tree(mk.plain(got), want)
    close_tree(mk.plain(er.calibration(probs.max(1), probs.argmax(1) == labels, 15)), json.loads(str(golden["calibration15"])))
    at = np.concatenate([[0], np.cumsum(mk.BATCHES)])
    batches = [(probs[a:b], preds[a:b], labels[a:b]) for a, b in zip(at[:-1], at[1:])]
    for m in (2, 100):
        close_tree(er.failures(batches, m), json.loads(str(golden[f"failures{m}"])))
    fails = json.loads(str(golden["failures100"]))
    assert [(f["batch_idx"], f["sample_idx"]) for f in fails] == [(0, 4), (1, 0), (2, 2)], "the wrong cells straddle the batch boundary"
    # every confidence is far enough from a bin edge that a forward differing in the last bits keeps the counts
    for n_bins in (10, 15):
        assert np.abs(probs.max(1)[:, None] - np.linspace(0, 1, n_bins + 1)[None]).min() > 1e-3


def test_float64_softmax_matches_the_reference_probabilities(golden):
    """per_cell's float64 softmax of the golden model's logits is the reference's f32 F.softmax to f32 rounding; its nll is torch's."""
    g3 = np.load(os.path.join(HERE, "golden", "model_v3_se.npz"))
    logits, labels = g3["logits"][:13], golden["labels"]
    r = er.per_cell(logits, labels)
    assert np.abs(r["p"] - golden["probabilities"]).max() < 4e-7 and (r["pred"] == golden["predictions"]).all()
    want = torch.nn.functional.cross_entropy(torch.from_numpy(logits).double(), torch.from_numpy(labels), reduction="none").numpy()
    assert np.abs(r["nll"] - want).max() < 1e-12
    ev = json.loads(str(golden["evaluate"]))
    at = np.concatenate([[0], np.cumsum(mk.BATCHES)])
    loss, acc, per_class = er.train_evaluate([(logits[a:b], labels[a:b]) for a, b in zip(at[:-1], at[1:])])
    assert loss == pytest.approx(ev["loss"], rel=1e-6) and acc == ev["accuracy"] and {str(k): float(v) for k, v in per_class.items()} == ev["per_class_acc"]


def test_restatement_matches_the_imported_reference():
    """compute_calibration and evaluate_dataset imported from the reference tree, on a tiny torch-CPU model and loader."""
    root = os.environ.get("SV_REFERENCE_ROOT", mk.DEFAULT_ROOT)
    try:
        ev, _, _ = mk.reference_modules(root)
    except FileNotFoundError:
        pytest.skip("no reference tree here")
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(784, 10)).eval()
    rs = np.random.RandomState(4)
    loader = [(torch.from_numpy(rs.randn(b, 1, 28, 28).astype(np.float32) * 3), torch.from_numpy(rs.randint(0, 10, b))) for b in (7, 7, 4)]
    want = ev.evaluate_dataset(model, loader, torch.device("cpu"), "tiny")
    with torch.no_grad():
        logits = torch.cat([model(d) for d, _ in loader]).numpy()
    labels = np.concatenate([t.numpy() for _, t in loader])
    r = er.per_cell(logits, labels)
    got = er.dataset_metrics(r["p"].astype(np.float32), r["pred"], labels, "tiny")
    close_tree(mk.plain(got), mk.plain(want))
    assert (got["predictions"] == want["predictions"]).all() and np.abs(got["probabilities"] - want["probabilities"]).max() < 4e-7
    for n_bins in er.BIN_COUNTS:
        close_tree(mk.plain(er.calibration(want["probabilities"].max(1), want["predictions"] == labels, n_bins)),
                   mk.plain(ev.compute_calibration(want["probabilities"], labels, n_bins)))


def test_aggregates_agree_with_the_quoted_lines():
    """aggregates (integers, fixed point) against calibration / per_class (the reference's lines) on the same per-cell values."""
    z, labels = er.random_cells(1.0)
    z, labels = z[:2000], labels[:2000]
    r = er.per_cell(z, labels)
    conf = r["conf"].astype(np.float32)
    for n_bins in er.BIN_COUNTS:
        agg = er.aggregates(r["pred"], conf, labels, n_bins)
        cal = er.calibration(conf, r["correct"], n_bins)
        assert [c for c in agg["bin_count"] if c] == cal["bin_counts"] and sum(agg["bin_count"]) == 2000
        assert er.ece_of(agg) == pytest.approx(cal["ece"], rel=1e-5)
        assert agg["n"] == 2000 and agg["n_correct"] == int(r["correct"].sum()) == agg["tot_count"][1] and agg["n_wrong"] == agg["tot_count"][2]
        assert agg["tot_conf"][0] == agg["tot_conf"][1] + agg["tot_conf"][2] == sum(int(float(c) * er.CONF_ONE) for c in conf)
    cm = np.array(agg["confusion"])
    pc = er.per_class(r["pred"], labels)
    assert all(pc[c]["support"] == cm[c].sum() and pc[c]["accuracy"] == cm[c, c] / cm[c].sum() for c in pc)
    # conf >= 2^-7 always, so conf * 2^30 is an integer: the fixed-point sum is the exact sum
    assert (conf >= 0.1 - 1e-7).all() and all(float(c) * er.CONF_ONE == int(float(c) * er.CONF_ONE) for c in conf)


@pytest.mark.parametrize("scale", er.SCALES)
def test_random_cells_are_what_the_gpu_tests_need(scale):
    """Both outcomes and every class occur in every batch size that can hold them; the cells test 1 drops from the pred comparison (top-2
    logit gap below the launch's absolute tolerance) stay under 1 %, on the reference alone."""
    z, labels = er.random_cells(scale)
    assert er.SIZES[-1] == 1024 * 256 + 2 and 257 in er.SIZES and 1 in er.SIZES
    for B in er.SIZES:
        r = er.per_cell(z[:B], labels[:B])
        t = torch.softmax(torch.from_numpy(z[:B].copy()), 1).numpy().astype(np.float64)
        noise, _, tol = tk.bounds(r["p"], t)
        top2 = np.sort(z[:B].astype(np.float64), 1)[:, -2:]
        dropped = (top2[:, 1] - top2[:, 0]) < tol.max()
        assert dropped.mean() <= 0.01, (B, dropped.mean())
        if B >= 63:
            assert 0 < r["correct"].sum() < B and len(set(labels[:B].tolist())) == 10 and len(set(r["pred"].tolist())) == 10
        if B >= 257 and scale == 1.0:
            assert len([c for c in er.aggregates(r["pred"], r["conf"], labels[:B], 10)["bin_count"] if c]) >= 5 or B > 10000
    if scale == 30.0:
        assert (er.per_cell(z[:257], labels[:257])["conf"] == 1.0).sum() > 10, "scale 30 saturates: the closed top edge of the last bin is hit"


def test_crafted_cells_are_exact():
    z, labels, conf, pred = er.crafted_cells()
    r = er.per_cell(z, labels)
    assert (r["conf"] == conf).all() and (r["pred"] == pred).all(), "float64 agrees with the hand-derived values exactly"
    assert (np.exp(np.float32(-1000)) == 0) and sorted(set(conf.tolist())) == [0.25, 0.5, 1.0]
    agg = er.aggregates(pred, conf, labels, 10)
    assert agg["bin_count"] == [0, 0, 4, 0, 4, 0, 0, 0, 0, 8] and agg["bin_correct"] == [0, 0, 1, 0, 1, 0, 0, 0, 0, 6]
    assert er.ece_of(agg) == 0.125 + 0.0625 and agg["n_correct"] == 8
    assert er.per_cell(er.ALL_EQUAL[None], [0])["pred"][0] == 0 and float(np.float32(0.1)) > 0.1


def test_failure_cells_are_placed():
    z, labels, wrong = er.failure_cells()
    r = er.per_cell(z, labels)
    assert len(z) == 300 and len(wrong) == 40 and (np.nonzero(~r["correct"])[0] == wrong).all()
    assert {0, 254, 255, 256, 257, 299} <= set(wrong.tolist())
    p32 = r["p"].astype(np.float32)
    for i in wrong:
        top = np.sort(p32[i])[::-1][:4]
        if i == 255:
            order = np.argsort(-z[i], kind="stable")
            assert z[i][order[1]] == z[i][order[2]] and order[1] < order[2] and z[i][order[0]] > z[i][order[1]] > z[i][order[3]]
        else:
            assert top[0] > top[1] > top[2] > top[3], i


def test_edge_cells_are_edges():
    e = er.edge_cells()
    z, lab = e["no_support"]
    r = er.per_cell(z, lab)
    assert 7 not in lab and 7 not in r["pred"] and 7 not in er.per_class(r["pred"], lab) and 0 < r["correct"].sum() < len(lab)
    assert er.per_cell(*e["all_correct"])["correct"].all() and not er.per_cell(*e["all_wrong"])["correct"].any()
    z, lab = e["bad_labels"]
    assert sorted(lab[(lab < 0) | (lab > 9)].tolist()) == [-1, 10]
    z, lab = e["nonfinite"]
    assert np.isnan(z).sum() == 1 and np.isinf(z).sum() == 1 and (~np.isfinite(z)).any(1).sum() == 2


# ---- the inputs of tests/test_gpu_eval_modes.py ----------------------------------------------------------------------------------------------
def test_decimal_edges_fall_on_the_side_they_were_chosen_for():
    """f32(0.1) and f32(0.3) lie above the double edge of the same name, f32(0.7) below: comparing in float would move each cell."""
    edges, n_bins = er.EDGE_SETS["decimal"]
    assert n_bins == 4 and edges.dtype == np.float64 and edges.tolist() == [0, 0.1, 0.3, 0.7, 1.0]
    for v, above in ((0.1, True), (0.3, True), (0.7, False)):
        c = float(np.float32(v))
        print(f"f32({v}) = {c!r}: {'above' if c > v else 'below'} the double edge {v!r}")
        assert (c > v) == above and c != v and np.float32(v) == np.float32(c)
    for name, (edges, n_bins) in er.EDGE_SETS.items():
        assert len(edges) == n_bins + 1 and (np.diff(edges) >= 0).all() and 1 <= n_bins <= 64, name
    assert er.EDGE_SETS["uniform10"][0].tolist() == np.linspace(0, 1, 11).tolist() and er.EDGE_SETS["fine64"][1] == 64
    assert len(set(np.diff(er.EDGE_SETS["fine64"][0]).round(12).tolist())) == 64, "fine64 is not uniform"


def test_prob_cells_are_what_they_are_for():
    probs, labels, marks = er.prob_cells()
    r = er.per_cell_prob(probs, labels)
    f = np.float32
    assert probs.dtype == np.float32 and len(probs) == 2 * 257 + len(marks) and len(set(marks.values())) == len(marks) == 15
    soft = probs[:514]
    assert r["finite"][:514].all() and (soft[257:].max(1) == 1.0).sum() > 10, "scale 30 saturates"
    tiny = np.abs(soft[257:])
    assert (tiny == 0).any() and ((tiny > 0) & (tiny < 2.0 ** -126)).any(), "scale 30 gives zero and denormal entries"
    assert 0 < r["correct"][:514].sum() < 514

    def row(name):
        i = marks[name]
        return {k: v[i] for k, v in r.items()}, probs[i], int(labels[i])

    c, p, lab = row("tiny")
    assert c["finite"] and c["pred"] == 0 and int(float(c["conf"]) * er.CONF_ONE) == 0 and 0 < float(c["conf"]) <= 0.1
    c, p, lab = row("zeros")
    assert c["finite"] and c["pred"] == 0 == lab and c["conf"] == 0 and c["true_prob"] == 0 and c["nll"] == np.inf and c["correct"]
    c, p, lab = row("sub_unit")
    assert c["finite"] and float(c["conf"]) * er.CONF_ONE == 0.75
    c, p, lab = row("small")
    fx = float(c["conf"]) * er.CONF_ONE
    assert c["finite"] and fx - int(fx) > 0.5 and float(c["conf"]) < 2.0 ** -7, "rounding the fixed-point term would add one"
    c, p, lab = row("negatives")
    order = np.argsort(-p, kind="stable")[:3]
    assert c["finite"] and not c["correct"] and p.max() == f(0.6) and (np.delete(p, c["pred"]) <= -1).all() and (p >= -3).all()
    assert order.tolist() == [4, 1, 5] and p[1] == p[5] == -1.0 and c["true_prob"] < 0 and np.isnan(c["nll"])
    c, p, lab = row("neg_label")
    assert c["finite"] and not c["correct"] and c["true_prob"] < 0 and np.isnan(c["nll"]) and p.max() == f(0.9)
    c, p, lab = row("above_one")
    assert not c["finite"] and np.isfinite(p).all() and p.max() == np.nextafter(f(1), f(2)) > 1
    c, p, lab = row("neg_top")
    assert not c["finite"] and np.isfinite(p).all() and p.max() == f(-0.25) and c["pred"] == 5 and (np.delete(p, 5) < -0.25).all()
    c, p, lab = row("nan")
    assert not c["finite"] and np.isnan(p).sum() == 1 and c["pred"] == 3 != np.nanargmax(p), "np.argmax takes the NaN, not the largest number"
    c, p, lab = row("inf")
    assert not c["finite"] and np.isinf(p).sum() == 1 and c["pred"] == 6
    for name, top in (("on_0.1", f(0.1)), ("on_0.3", f(0.3)), ("on_0.7", f(0.7)), ("on_0.125", f(0.125)), ("below_0.5", np.nextafter(f(0.5), f(0)))):
        c, p, lab = row(name)
        assert c["finite"] and c["conf"] == top and (np.delete(p, c["pred"]) < top).all(), name
    assert f(0.125) == 0.125 and float(np.nextafter(f(0.5), f(0))) < 0.5
    wrong_valid = r["finite"] & ~r["correct"]
    assert {marks[k] for k in ("negatives", "neg_label", "on_0.3", "below_0.5")} <= set(np.nonzero(wrong_valid)[0].tolist())
    assert sorted(np.nonzero(~r["finite"])[0].tolist()) == sorted(marks[k] for k in ("above_one", "neg_top", "nan", "inf"))
    # where the crafted cells land: derived by hand from evaluate_v2.py:163, `conf > edges[i] and conf <= edges[i + 1]`
    where = {name: {} for name in er.EDGE_SETS}
    for name, (edges, n_bins) in er.EDGE_SETS.items():
        for k, i in marks.items():
            if r["finite"][i]:
                one = er.aggregates(r["pred"][i:i + 1], r["conf"][i:i + 1], labels[i:i + 1], n_bins, edges=edges)["bin_count"]
                where[name][k] = one.index(1) if 1 in one else None
    assert where["uniform10"]["tiny"] == 0 and where["uniform10"]["zeros"] is None and where["uniform10"]["on_0.1"] == 1 and where["uniform10"]["below_0.5"] == 4
    assert [where["decimal"][k] for k in ("on_0.1", "on_0.3", "on_0.7", "on_0.125", "negatives")] == [1, 2, 2, 1, 2]
    assert where["repeated"]["below_0.5"] == 0 and where["repeated"]["negatives"] == 3 and where["repeated"]["zeros"] is None
    assert where["inner"]["on_0.1"] is None and where["inner"]["on_0.3"] == 0 and where["inner"]["neg_label"] == 1
    assert where["one"]["on_0.125"] is None and where["one"]["on_0.1"] is None and where["one"]["on_0.3"] == 0
    for name, (edges, n_bins) in er.EDGE_SETS.items():
        agg = er.aggregates(r["pred"], r["conf"], labels, n_bins, finite=r["finite"], edges=edges)
        assert agg["nonfinite"] == 4 and agg["n"] == len(probs) - 4
        if name == "fine64":
            assert agg["bin_count"][63] > 10, "the last bin of fine64 holds the saturated cells: a missing last edge changes a count"
        if name == "repeated":
            assert agg["bin_count"][1] == agg["bin_count"][2] == 0 and agg["bin_count"][0] > 0 and agg["bin_count"][3] > 0
        if name == "inner":
            assert 0 < sum(agg["bin_count"]) < agg["n"] and (r["conf"][r["finite"]] < 0.2).any() and (r["conf"][r["finite"]] > 0.9).any()


def test_vectorised_aggregates_equal_the_loop():
    """aggregates_fast against aggregates on 3,000 logits cells at both scales, with bad labels and non-finite cells, and on prob_cells(),
    for every edge set and the default edges."""
    cases = []
    for scale in er.SCALES:
        z, labels = er.random_cells(scale)
        r = er.per_cell(z[:3000], labels[:3000])
        lab = labels[:3000].copy()
        lab[[7, 1500]] = [10, -1]
        finite = np.ones(3000, bool)
        finite[[3, 8, 2999]] = False
        cases.append((r["pred"], r["conf"].astype(np.float32), lab, finite))
    probs, labels, _ = er.prob_cells()
    r = er.per_cell_prob(probs, labels)
    cases.append((r["pred"], r["conf"], labels, r["finite"]))
    for pred, conf, lab, finite in cases:
        for name, (edges, n_bins) in er.EDGE_SETS.items():
            assert er.aggregates_fast(pred, conf, lab, n_bins, finite=finite, edges=edges) == er.aggregates(pred, conf, lab, n_bins, finite=finite, edges=edges), name
        for n_bins in er.BIN_COUNTS:
            assert er.aggregates_fast(pred, conf, lab, n_bins, finite=finite) == er.aggregates(pred, conf, lab, n_bins, finite=finite)


def test_long_list_cells_are_placed():
    z, labels, wrong = er.long_list_cells()
    assert len(z) == er.SIZES[-1] == 262146 and len(wrong) == 300 and (np.diff(wrong) > 0).all()
    pred = z.argmax(1)
    assert (np.nonzero(pred != labels)[0] == wrong).all() and ((labels >= 0) & (labels <= 9)).all()
    have = set(wrong.tolist())
    assert {0, 255, 256, 65535, 65536, 65791, 131071, 131072, 262143, 262144, 262145} <= have
    tile = wrong // 256
    assert (tile == er.LONG_TILE).sum() == 256 and er.LONG_TILE > 256, "one whole tile past the seam between scan chunks is wrong"
    assert (tile < 256).any() and ((tile >= 256) & (tile < 512)).any() and (tile == 1024).sum() == 2
    assert (tile >= 512).sum() > 5 and len(set(tile.tolist())) > 30
    assert (tile == 0).sum() != (tile == 1024).sum(), "workgroup 0's two tiles hold different counts"
