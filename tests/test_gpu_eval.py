"""GPU (-m gpu): K21 (csrc/k21_eval.hip) through Context.eval_metrics, and the ml/evaluate_v2.py drop-in, against tests/eval_ref.py.

1 per cell      probs, conf, true_prob (and nll by the same rule on its own noise) within the bound tests/test_gpu_softmax_topk.py applies
                (its bounds(), C_ABS = C_REL = 4, reused as it stands); pred exact but for cells whose top-2 logit gap is below that
                bound; probs bit-identical to Context.softmax_topk(k = 10)
2 aggregates    from the kernel's own pred / conf / correct, the restatement's integers exactly (n_bins 1, 10, 15, 64)
3 end to end    crafted logits whose f32 softmax is known: constants derived by hand below
4 launch shape  4,097 cells in one call and in 17 uneven accumulating calls: the same bytes
5 failures      the first min(max_failures, 40) wrong cells in index order; ties lowest class first
6 edges         no support, all correct, all wrong, bad labels, NaN / Inf, int32 labels, temperatures, NULL outputs
7 drop-in       evaluate_dataset, compute_calibration, find_failures, evaluate against tests/golden/eval_goldens.npz
8 streams       the asynchronous entry behind a late copy on a busy side stream, and captured once and replayed

Every test fails on the parent commit: Context has no eval_metrics there."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import cnn_oracle
import eval_ref as er
import model_v3_ref
import test_gpu_softmax_topk as tk

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ALL = ("probs", "pred", "conf", "true_prob", "nll", "correct")


def dev(ctx, a):
    return torch.from_numpy(np.array(a)).to(ctx.device)                      # a copy: the shared inputs are not writable


def run(ctx, z, labels, **kw):
    out, agg = ctx.eval_metrics(dev(ctx, z), dev(ctx, labels), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, agg


_REF = {}


def reference(scale, B, temperature=1.0):
    """per_cell of the first B random cells at `scale`, the torch CPU f32 softmax and nll that give the noise, once per key."""
    key = (scale, B, temperature)
    if key not in _REF:
        z, labels = er.random_cells(scale)
        z, labels = z[:B], labels[:B]
        r = er.per_cell(z, labels, temperature)
        zt = torch.from_numpy(z.copy()) / temperature
        r["t"] = torch.softmax(zt, 1).numpy().astype(np.float64)
        r["t_nll"] = torch.nn.functional.cross_entropy(zt, torch.from_numpy(labels.copy()), reduction="none").numpy().astype(np.float64)
        r["z"], r["labels"] = z, labels
        _REF[key] = r
    return _REF[key]


def check_per_cell(out, r, what):
    """Test 1's comparison of one launch's per-cell outputs with the float64 restatement r."""
    B = len(r["z"])
    rows = np.arange(B)
    noise, rel_noise, tol = tk.bounds(r["p"], r["t"])
    err = np.abs(out["probs"].astype(np.float64) - r["p"])
    print(f"{what}: max|probs - f64| {err.max():.3e}, noise {noise:.3e}, largest err / bound {(err / tol).max():.3f}")
    assert (err <= tol).all()
    top2 = np.sort(r["z"].astype(np.float64), 1)[:, -2:]
    kept = (top2[:, 1] - top2[:, 0]) >= tol.max()
    assert 1 - kept.mean() <= 0.01
    assert (out["pred"][kept] == r["pred"][kept]).all()
    same = out["pred"] == r["pred"]
    assert (np.abs(out["conf"].astype(np.float64) - r["conf"]) <= tol[rows, r["pred"]])[same].all()
    assert (np.abs(out["true_prob"].astype(np.float64) - r["true_prob"]) <= tol[rows, r["labels"]]).all()
    nll_noise = np.abs(r["t_nll"] - r["nll"]).max()
    nll_tol = cnn_oracle.tolerance(r["nll"], nll_noise, tk.C_ABS)
    nll_err = np.abs(out["nll"].astype(np.float64) - r["nll"]).max()
    print(f"{what}: max|nll - f64| {nll_err:.3e}, noise {nll_noise:.3e}, bound {nll_tol:.3e}")
    assert nll_err <= nll_tol
    assert (out["correct"].astype(bool) == (out["pred"] == r["labels"])).all()
    assert out["conf"].tobytes() == out["probs"][rows, out["pred"]].tobytes() and out["true_prob"].tobytes() == out["probs"][rows, r["labels"]].tobytes()


@pytest.mark.parametrize("scale", er.SCALES)
@pytest.mark.parametrize("B", er.SIZES)
def test_per_cell_and_aggregates(ctx, B, scale):
    """Tests 1 and 2 on one launch per n_bins."""
    r = reference(scale, B)
    zd, ld = dev(ctx, r["z"]), dev(ctx, r["labels"])
    first = None
    for n_bins in er.BIN_COUNTS:
        out, agg = ctx.eval_metrics(zd, ld, n_bins=n_bins, want=ALL)
        out = {k: v.cpu().numpy() for k, v in out.items()}
        if first is None:
            first = out
            check_per_cell(out, r, f"B {B} scale {scale}")
            idx, prob = ctx.softmax_topk(zd, 10)
            idx, prob = idx.cpu().numpy().astype(np.int64), prob.cpu().numpy()
            assert np.take_along_axis(out["probs"], idx, 1).tobytes() == prob.tobytes(), "probs are not bit-identical to softmax_topk's"
        else:
            assert all(out[k].tobytes() == first[k].tobytes() for k in ALL)
        if B <= 10000:
            assert agg == er.aggregates(out["pred"], out["conf"], r["labels"], n_bins), (B, scale, n_bins)
            continue
        # the large size: the same integers from numpy, not from the restatement's Python loop over the cells
        fx = (out["conf"].astype(np.float64) * er.CONF_ONE).astype(np.int64)
        ok = out["correct"].astype(bool)
        edges = np.linspace(0, 1, n_bins + 1)
        c = out["conf"].astype(np.float64)
        for b in range(n_bins):
            m = (c > edges[b]) & (c <= edges[b + 1])
            assert (agg["bin_count"][b], agg["bin_correct"][b], agg["bin_conf"][b]) == (int(m.sum()), int((m & ok).sum()), int(fx[m].sum()))
        cm = np.zeros((10, 10), np.int64)
        np.add.at(cm, (r["labels"], out["pred"].astype(np.int64)), 1)
        assert agg["confusion"] == cm.tolist() and (agg["n"], agg["n_correct"], agg["n_wrong"], agg["bad_labels"], agg["nonfinite"]) == (B, int(ok.sum()), int((~ok).sum()), 0, 0)
        assert agg["tot_conf"] == [int(fx.sum()), int(fx[ok].sum()), int(fx[~ok].sum())] and agg["tot_count"] == [B, int(ok.sum()), int((~ok).sum())]


def test_crafted_logits_end_to_end(ctx):
    """Test 3.  By hand: 8 one-hot cells (conf 1.0, the closed top edge of bin 9; 6 correct), 4 two-way ties (0.5, the closed top edge of
    bin 4; 1 correct), 4 four-way ties (0.25, bin 2; 1 correct).  ECE = |6/8 - 1| * 8/16 + |1/4 - 1/2| * 4/16 + |1/4 - 1/4| * 4/16 = 0.1875."""
    z, labels, _, _ = er.crafted_cells()
    out, agg = run(ctx, z, labels, want=ALL)
    assert out["conf"].tolist() == [1.0] * 8 + [0.5] * 4 + [0.25] * 4
    assert out["pred"].tolist() == [0, 1, 2, 3, 5, 7, 8, 9, 2, 0, 4, 7, 1, 0, 6, 3], "a tie goes to its lowest class"
    assert out["true_prob"][[9, 10, 11]].tolist() == [0.5] * 3 and out["true_prob"][1] == 0.0 and out["nll"][1] == 1000.0 and out["nll"][0] == 0.0
    assert agg["bin_count"] == [0, 0, 4, 0, 4, 0, 0, 0, 0, 8] and agg["bin_correct"] == [0, 0, 1, 0, 1, 0, 0, 0, 0, 6]
    assert agg["bin_conf"] == [0, 0, 1 << 30, 0, 2 << 30, 0, 0, 0, 0, 8 << 30]
    assert (agg["n"], agg["n_correct"], agg["n_wrong"], agg["bad_labels"], agg["nonfinite"]) == (16, 8, 8, 0, 0)
    assert agg["tot_count"] == [16, 8, 8] and agg["tot_correct"] == [8, 8, 0] and agg["tot_conf"] == [11 << 30, (6 << 30) + (1 << 29) + (1 << 28), (4 << 30) + (1 << 28)]
    assert er.ece_of(agg) == 0.1875
    cm = np.array(agg["confusion"])
    assert cm.sum() == 16 and np.trace(cm) == 8 and cm[4, 1] == 1 and cm[9, 0] == 2
    # the all-equal cell: its conf is whatever 1 / den rounds to; it has to be in the bin the restatement puts that conf in, and pred 0
    out, agg = run(ctx, np.concatenate([z, er.ALL_EQUAL[None]]), np.concatenate([labels, [0]]), want=ALL)
    assert out["pred"][16] == 0 and out["correct"][16] == 1 and (out["probs"][16] == out["conf"][16]).all()
    assert agg == er.aggregates(out["pred"], out["conf"], np.concatenate([labels, [0]]), 10)
    print("all-equal cell: conf", repr(float(out["conf"][16])), "bins", agg["bin_count"])


def test_launch_shape_independence(ctx):
    """Test 4."""
    z, labels = er.random_cells(1.0)
    z, labels = dev(ctx, z[:4097]), dev(ctx, labels[:4097])
    one, _ = ctx.eval_metrics(z, labels, n_bins=15, max_failures=50)
    sizes = [1, 255, 256, 257, 3, 511, 64, 300, 1000, 2, 129, 700, 31, 257, 90, 200, 41]
    assert len(sizes) == 17 and sum(sizes) == 4097
    stats, fails, at = ctx.eval_stats_buffer(), None, 0
    for k, b in enumerate(sizes):
        out, _ = ctx.eval_metrics(z[at:at + b], labels[at:at + b], n_bins=15, max_failures=50, stats=stats, failures=fails, accumulate=True, index_base=at,
                                  read_back=False)
        fails = out["failures"]
        at += b
    torch.cuda.synchronize()
    assert one["stats"].cpu().numpy().tobytes() == stats.cpu().numpy().tobytes()
    assert one["failures"].cpu().numpy().tobytes() == fails.cpu().numpy().tobytes()


@pytest.mark.parametrize("max_failures", [0, 1, 39, 40, 100])
def test_failure_list(ctx, max_failures):
    """Test 5."""
    z, labels, wrong = er.failure_cells()
    out, agg = ctx.eval_metrics(dev(ctx, z), dev(ctx, labels), max_failures=max_failures, want=("probs",))
    assert agg["n_wrong"] == 40 and agg["n"] == 300
    if max_failures == 0:
        assert "failures" not in out
        return
    n = min(max_failures, 40)
    rec = ctx.eval_failures(out["failures"], n)
    probs = out["probs"].cpu().numpy()
    assert rec["index"].tolist() == wrong[:n].tolist()
    assert rec["label"].tolist() == labels[wrong[:n]].tolist() and rec["pred"].tolist() == z[wrong[:n]].argmax(1).tolist()
    for f in rec:
        p = probs[f["index"]]
        order = np.argsort(-p, kind="stable")[:3]                          # stable: equal probabilities lowest class first
        assert f["top3_index"].tolist() == order.tolist() and f["top3_prob"].tobytes() == p[order].tobytes()
        assert f["conf"] == p[f["pred"]] and f["true_prob"] == p[f["label"]] and f["top3_index"][0] == f["pred"]
        if f["index"] == 255:
            assert f["top3_prob"][1] == f["top3_prob"][2] and f["top3_index"][1] < f["top3_index"][2]


def test_edges(ctx):
    """Test 6."""
    import sudoku_vision_amd as sva
    e = er.edge_cells()
    out, agg = run(ctx, *e["no_support"], want=("pred", "conf"))
    assert agg == er.aggregates(out["pred"], out["conf"], e["no_support"][1], 10) and sum(agg["confusion"][7]) == 0
    out, agg = run(ctx, *e["all_correct"], want=("pred", "conf"))
    assert agg["n_wrong"] == 0 and agg["tot_count"] == [90, 90, 0] and agg["tot_conf"][2] == 0 and agg["tot_conf"][0] == agg["tot_conf"][1]
    out, agg = run(ctx, *e["all_wrong"], want=("pred", "conf"))
    assert agg["n_correct"] == 0 and agg["tot_count"] == [90, 0, 90] and agg["tot_conf"][1] == 0 and agg["bin_correct"] == [0] * 10
    # labels 10 and -1: the read-back form refuses, the block still holds the other 88 cells
    z, bad = e["bad_labels"]
    stats = ctx.eval_stats_buffer()
    with pytest.raises(sva._native.NativeError, match="SV_ERR_BAD_ARG"):
        ctx.eval_metrics(dev(ctx, z), dev(ctx, bad), stats=stats)
    out, none = ctx.eval_metrics(dev(ctx, z), dev(ctx, bad), stats=stats, read_back=False, want=ALL)
    assert none is None
    agg = ctx.eval_stats_dict(stats, 10)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert agg["bad_labels"] == 2 and agg["n"] == 88 and agg == er.aggregates(out["pred"], out["conf"], bad, 10)
    assert np.isnan(out["true_prob"][[10, 80]]).all() and np.isnan(out["nll"][[10, 80]]).all() and not out["correct"][[10, 80]].any()
    # one NaN and one Inf cell: counted as such and nowhere else
    zn, lab = e["nonfinite"]
    out, agg = run(ctx, zn, lab, want=ALL, max_failures=90)
    finite = np.isfinite(zn).all(1)
    assert agg["nonfinite"] == 2 and agg["n"] == 88 and sum(agg["bin_count"]) == 88 and sum(map(sum, agg["confusion"])) == 88
    assert agg == er.aggregates(out["pred"], out["conf"], lab, 10, finite=finite) and not out["correct"][~finite].any()
    good, agg_good = run(ctx, zn[finite], lab[finite], want=ALL, max_failures=90)
    assert all(out[k][finite].tobytes() == good[k].tobytes() for k in ALL) and {**agg, "nonfinite": 0} == agg_good
    rec, rec_good = ctx.eval_failures(torch.from_numpy(out["failures"]), agg["n_wrong"]), ctx.eval_failures(torch.from_numpy(good["failures"]), agg["n_wrong"])
    assert rec["index"].tolist() == np.nonzero(finite)[0][rec_good["index"]].tolist() and len(rec) == agg["n_wrong"] > 0
    # int32 labels, NULL outputs
    z, lab = e["mixed"]
    out64, agg64 = run(ctx, z, lab, want=ALL)
    out32, agg32 = run(ctx, z, lab.astype(np.int32), want=ALL)
    none, agg0 = run(ctx, z, lab, want=())
    assert agg64 == agg32 == agg0 and set(none) == {"stats"} and all(out64[k].tobytes() == out32[k].tobytes() for k in ALL)
    for k in ALL:                                                          # each output alone
        one, _ = run(ctx, z, lab, want=(k,))
        assert one[k].tobytes() == out64[k].tobytes()
    # temperatures
    for T in (0.5, 2.0):
        r = reference(1.0, 257, T)
        out, agg = run(ctx, r["z"], r["labels"], temperature=T, want=ALL)
        check_per_cell(out, r, f"T {T}")
        assert agg == er.aggregates(out["pred"], out["conf"], r["labels"], 10)
    with pytest.raises(sva._native.NativeError, match="SV_ERR_BAD_ARG"):
        ctx.eval_metrics(dev(ctx, z), dev(ctx, lab), temperature=0.0)
    with pytest.raises(sva._native.NativeError, match="SV_ERR_BAD_ARG"):
        ctx.eval_metrics(dev(ctx, z), dev(ctx, lab), n_bins=65)


def close(got, want, tol):
    """Same keys and kinds; counts exact; floats within tol."""
    if isinstance(want, dict):
        assert [str(k) for k in got] == [str(k) for k in want], (list(got), list(want))
        for g, w in zip(got.values(), want.values()):
            close(g, w, tol)
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want)
        for g, w in zip(got, want):
            close(g, w, tol)
    elif isinstance(want, float):
        assert isinstance(got, (float, np.floating)) and abs(float(got) - want) <= tol, (got, want, tol)
    else:
        assert type(got) is type(want) and got == want, (got, want)


def test_dropin_against_goldens(ctx):
    """Test 7: DigitCNNv3 with the seeded weights of tests/golden/model_v3_se.npz on a loader of 5, 5 and 3 cells."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_eval_goldens as mk
    sys.path.pop(0)
    import sudoku_vision_amd as sva
    ml = os.path.join(os.path.dirname(sva.__file__), "ml")
    sys.path.insert(0, ml)
    try:
        for name in ("evaluate_v2", "model_v3"):
            sys.modules.pop(name, None)
        import evaluate_v2 as ev
        from model_v3 import DigitCNNv3
    finally:
        sys.path.remove(ml)
    golden = np.load(os.path.join(HERE, "golden", "eval_goldens.npz"))
    g3 = np.load(os.path.join(HERE, "golden", "model_v3_se.npz"))
    model = DigitCNNv3(use_se=True)
    model.load_state_dict(model_v3_ref.random_state_dict_v3(int(g3["w_seed"]), True), strict=False)
    model = model.to(ctx.device).eval()
    x, labels = mk.inputs(g3)
    loader = mk.loader_of(x, labels)
    # the tolerance of test 1 for these 13 cells: bounds() on the reference's probabilities
    p64 = er.per_cell(g3["logits"][:13], labels)["p"]
    noise, _, tol = tk.bounds(p64, golden["probabilities"].astype(np.float64))
    tol = float(tol.max())
    res = ev.evaluate_dataset(model, loader, ctx.device, "golden")
    want = json.loads(str(golden["dataset"]))
    err = np.abs(res["probabilities"].astype(np.float64) - golden["probabilities"]).max()
    print(f"drop-in: max|probabilities - reference| {err:.3e}, bound {tol:.3e} (softmax noise {noise:.3e})")
    assert list(res) == list(want) + ["predictions", "labels", "probabilities"]
    for k in ("predictions", "labels", "probabilities"):
        assert res[k].dtype == golden[k].dtype and res[k].shape == golden[k].shape
    assert (res["predictions"] == golden["predictions"]).all() and (res["labels"] == golden["labels"]).all()
    assert all(type(v) is np.float32 for v in res["calibration"]["bin_confidences"]) and all(type(v) is np.float64 for v in res["calibration"]["bin_accuracies"])
    close(mk.plain(res), want, tol)
    assert err <= tol
    cal = ev.compute_calibration(golden["probabilities"], golden["labels"], 15)
    close(mk.plain(cal), json.loads(str(golden["calibration15"])), tol)
    for m in (2, 100):
        fails = ev.find_failures(model, loader, ctx.device, m)
        want_f = json.loads(str(golden[f"failures{m}"]))
        assert [(f["batch_idx"], f["sample_idx"]) for f in fails] == [(f["batch_idx"], f["sample_idx"]) for f in want_f]
        for f, w in zip(fails, want_f):
            assert (f["image"] == x[sum(mk.BATCHES[:f["batch_idx"]]) + f["sample_idx"]]).all() and f["image"].shape == (1, 28, 28)
            close({k: v for k, v in f.items() if k != "image"}, w, tol)
    want_e = json.loads(str(golden["evaluate"]))
    loss, acc, per_class = ev.evaluate(model, loader, torch.nn.CrossEntropyLoss(), ctx.device)
    nll64 = er.per_cell(g3["logits"][:13], labels)["nll"]
    nll_tol = cnn_oracle.tolerance(nll64, np.abs(torch.nn.functional.cross_entropy(torch.from_numpy(g3["logits"][:13]), torch.from_numpy(labels), reduction="none").numpy() - nll64).max(), tk.C_ABS)
    print(f"drop-in: loss {loss!r} reference {want_e['loss']!r} bound {nll_tol:.3e}")
    assert abs(loss - want_e["loss"]) <= nll_tol and acc == want_e["accuracy"] and {str(k): float(v) for k, v in per_class.items()} == want_e["per_class_acc"]
    with pytest.raises(NotImplementedError, match="CrossEntropyLoss"):
        ev.evaluate(model, loader, torch.nn.CrossEntropyLoss(label_smoothing=0.1), ctx.device)
    with pytest.raises(NotImplementedError):
        ev.evaluate(model, loader, torch.nn.NLLLoss(), ctx.device)


def test_dropin_takes_the_other_models(ctx):
    """DigitCNN and DigitCNNv3Light through evaluate_dataset: the counts are those of the restatement on the model's own logits."""
    import sudoku_vision_amd as sva
    ml = os.path.join(os.path.dirname(sva.__file__), "ml")
    sys.path.insert(0, ml)
    try:
        for name in ("evaluate_v2", "model_v3", "model"):
            sys.modules.pop(name, None)
        import evaluate_v2 as ev
        from model import DigitCNN
        from model_v3 import DigitCNNv3Light
    finally:
        sys.path.remove(ml)
    rs = np.random.RandomState(9)
    x = rs.uniform(-1, 1, (13, 1, 28, 28)).astype(np.float32)
    for cls in (DigitCNN, DigitCNNv3Light):
        torch.manual_seed(1)
        model = cls().to(ctx.device).eval()
        with torch.no_grad():
            logits = model(dev(ctx, x)).cpu().numpy()
        labels = np.where(np.arange(13) % 3 == 0, (logits.argmax(1) + 1) % 10, logits.argmax(1)).astype(np.int64)
        loader = [(torch.from_numpy(x[a:b]), torch.from_numpy(labels[a:b])) for a, b in ((0, 5), (5, 10), (10, 13))]
        res = ev.evaluate_dataset(model, loader, ctx.device, cls.__name__)
        want = er.dataset_metrics(res["probabilities"], res["predictions"], labels, cls.__name__)
        assert res["samples"] == 13 and res["accuracy"] == want["accuracy"] == 8 / 13 and list(res["per_class"]) == list(want["per_class"])
        assert res["calibration"]["bin_counts"] == want["calibration"]["bin_counts"]
        assert res["calibration"]["ece"] == pytest.approx(want["calibration"]["ece"], rel=1e-5)


class TestStreams:
    """Test 8, in the pattern of tests/test_gpu_stream_order.py: the buffers hold A; on a side stream a delay, the copy of B and the
    asynchronous entry are enqueued with no synchronisation between them, and the result must be B's.  Then the call is captured once
    and replayed on B, on A, and on A again."""

    @pytest.fixture(scope="class")
    def env(self, ctx):
        s = torch.cuda.Stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)
            a.record()
            torch.cuda._sleep(20_000_000)
            b.record()
        s.synchronize()
        cycles_per_ms = 20_000_000 / a.elapsed_time(b)
        z, labels = er.random_cells(1.0)
        A = (z[:600], labels[:600])
        B = (z[600:1200], labels[600:1200])
        want = {}
        for name, (zz, ll) in (("A", A), ("B", B)):
            out, _ = ctx.eval_metrics(dev(ctx, zz), dev(ctx, ll), n_bins=15, max_failures=20, want=ALL)
            torch.cuda.synchronize()
            want[name] = {k: v.cpu().numpy().tobytes() for k, v in out.items()}
        assert want["A"]["stats"] != want["B"]["stats"] and want["A"]["failures"] != want["B"]["failures"]
        return {"s": s, "delay": int(5.0 * cycles_per_ms), "A": tuple(dev(ctx, v) for v in A), "B": tuple(dev(ctx, v) for v in B), "want": want}

    @staticmethod
    def same(out, want, what):
        for k, v in want.items():
            assert out[k].cpu().numpy().tobytes() == v, f"{what}: {k} differs"

    def test_behind_a_late_copy_on_a_side_stream(self, ctx, env):
        z, labels = env["A"][0].clone(), env["A"][1].clone()
        stats, fails = ctx.eval_stats_buffer(), torch.zeros((20, 48), dtype=torch.uint8, device=ctx.device)
        torch.cuda.synchronize()
        with torch.cuda.stream(env["s"]):
            torch.cuda._sleep(env["delay"])
            z.copy_(env["B"][0], non_blocking=True)
            labels.copy_(env["B"][1], non_blocking=True)
            out, _ = ctx.eval_metrics(z, labels, n_bins=15, max_failures=20, want=ALL, stats=stats, failures=fails, read_back=False)
        env["s"].synchronize()
        self.same(out, env["want"]["B"], "behind a late copy of B")
        torch.cuda.synchronize()

    @pytest.mark.parametrize("accumulate", [False, True])
    def test_capture_once_and_replay(self, ctx, env, accumulate):
        z, labels = env["A"][0].clone(), env["A"][1].clone()
        stats, fails = ctx.eval_stats_buffer(), torch.zeros((20, 48), dtype=torch.uint8, device=ctx.device)
        ctx.eval_metrics(z, labels, n_bins=15, max_failures=20, want=ALL, read_back=False)       # warm-up at this shape: scratch, code objects
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=env["s"]):
                out, _ = ctx.eval_metrics(z, labels, n_bins=15, max_failures=20, want=ALL, stats=stats, failures=fails, accumulate=accumulate, read_back=False)
        except Exception:
            torch.cuda.synchronize()
            raise
        total = np.zeros(stats.numel(), np.int64)
        for step, which in enumerate(("B", "A", "A")):
            if step < 2:
                z.copy_(env[which][0], non_blocking=True)
                labels.copy_(env[which][1], non_blocking=True)
            g.replay()
            torch.cuda.synchronize()
            want = dict(env["want"][which])
            if accumulate:                                                 # the block adds up over the replays; the list is the first 20 since the clear
                total += np.frombuffer(want.pop("stats"), np.int64)
                assert (stats.cpu().numpy() == total).all(), f"replay {step}: the block is not the sum of the replays"
                want["failures"] = env["want"]["B"]["failures"]
            self.same(out, want, f"replay {step} on {which}, accumulate {accumulate}")
        del g
