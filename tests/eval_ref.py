"""CPU yardstick for K21 (csrc/k21_eval.hip, Context.eval_metrics) and the ml/evaluate_v2.py drop-in.  TEST INFRASTRUCTURE ONLY.

Written from the reference's ml/evaluate_v2.py and ml/train.py, not from the kernel: the softmax in float64, everything else as the quoted
lines do it.

  per_cell            softmax(logits / T) in float64, argmax of the logits (np.argmax: first maximum), conf, true_prob, nll
  calibration         ml/evaluate_v2.py:150-181 from the largest probabilities and the correct flags
  per_class           ml/evaluate_v2.py:104-125 from predictions and labels
  dataset_metrics     ml/evaluate_v2.py:96-147 from probabilities, predictions and labels: the dictionary evaluate_dataset returns
  failures            ml/evaluate_v2.py:194-220 from per-batch probabilities
  train_evaluate      ml/train.py:157-190 from per-batch logits
  aggregates          sv_eval_stats as Context.eval_stats_dict shows it, in Python integers, from per-cell pred / conf / labels
  aggregates_fast     the same dictionary from np.searchsorted and np.bincount, for the large size
  per_cell_prob       the probability-input mode: pred, conf, true_prob from the given f32 rows, nll = -log in float64, the finite rule

and the inputs the GPU tests use (tests/test_eval_ref.py checks each does what it was built for)."""
import numpy as np

CONF_ONE = 1 << 30
SIZES = (1, 63, 64, 65, 257, 1024 * 256 + 2)      # 1024 workgroups of 256 cells: above that a workgroup takes a second tile
SCALES = (1.0, 30.0)
BIN_COUNTS = (1, 10, 15, 64)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def per_cell(logits, labels, temperature=1.0):
    """logits f32 [B,10], labels int [B] in 0..9 -> dict: p f64 [B,10], pred, conf, true_prob, nll (f64), correct (bool)."""
    z = np.asarray(logits, np.float32).astype(np.float64) / float(temperature)
    labels = np.asarray(labels).astype(np.int64)
    m = z.max(1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(z - m)
        den = e.sum(1, keepdims=True)
        p = e / den
        lse = (m + np.log(den))[:, 0]
    rows = np.arange(len(z))
    pred = np.argmax(np.asarray(logits, np.float32), 1)
    return {"p": p, "pred": pred, "conf": p[rows, pred], "true_prob": p[rows, labels], "nll": lse - z[rows, labels], "correct": pred == labels}


def calibration(max_probs, accuracies, n_bins=10):
    """compute_calibration, ml/evaluate_v2.py:156-181, from probs.max(axis=1) and predictions == labels."""
    max_probs, accuracies = np.asarray(max_probs), np.asarray(accuracies, bool)
    bin_boundaries = np.linspace(0, 1, n_bins + 1)
    out = {"bin_centers": [], "bin_accuracies": [], "bin_confidences": [], "bin_counts": []}
    for i in range(n_bins):
        in_bin = (max_probs > bin_boundaries[i]) & (max_probs <= bin_boundaries[i + 1])
        if in_bin.sum() > 0:
            out["bin_centers"].append((bin_boundaries[i] + bin_boundaries[i + 1]) / 2)
            out["bin_accuracies"].append(accuracies[in_bin].mean())
            out["bin_confidences"].append(max_probs[in_bin].mean())
            out["bin_counts"].append(int(in_bin.sum()))
    ece = 0
    for acc, conf, count in zip(out["bin_accuracies"], out["bin_confidences"], out["bin_counts"]):
        ece += abs(acc - conf) * count / len(accuracies)
    out["ece"] = float(ece)
    return out


def per_class(preds, labels):
    """ml/evaluate_v2.py:104-125."""
    preds, labels = np.asarray(preds), np.asarray(labels)
    correct = preds == labels
    out = {}
    for cls in range(10):
        mask = labels == cls
        if mask.sum() == 0:
            continue
        tp = ((preds == cls) & (labels == cls)).sum()
        fp = ((preds == cls) & (labels != cls)).sum()
        fn = ((preds != cls) & (labels == cls)).sum()
        precision = tp / (tp + fp) if (tp + fp) > 0 else 0
        recall = tp / (tp + fn) if (tp + fn) > 0 else 0
        f1 = 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0
        out[cls] = {"precision": float(precision), "recall": float(recall), "f1": float(f1), "support": int(mask.sum()), "accuracy": float(correct[mask].mean())}
    return out


def dataset_metrics(probs, preds, labels, dataset_name="test"):
    """What evaluate_dataset returns (ml/evaluate_v2.py:96-147) for the gathered probabilities, predictions and labels."""
    probs, preds, labels = np.asarray(probs), np.asarray(preds), np.asarray(labels)
    correct = preds == labels
    max_probs = probs.max(axis=1)
    return {"dataset": dataset_name, "samples": len(labels), "accuracy": float(np.mean(correct)), "per_class": per_class(preds, labels),
            "mean_confidence": float(max_probs.mean()),
            "correct_confidence": float(max_probs[correct].mean() if correct.sum() > 0 else 0),
            "incorrect_confidence": float(max_probs[~correct].mean() if (~correct).sum() > 0 else 0),
            "calibration": calibration(max_probs, probs.argmax(axis=1) == labels, 10), "predictions": preds, "labels": labels, "probabilities": probs}


def failures(batches, max_failures=100):
    """find_failures (ml/evaluate_v2.py:194-220) without the image: batches = [(probs [b,10], preds [b], labels [b]), ...].  top-3: a
    stable descending sort, equal probabilities lowest class first."""
    out = []
    for batch_idx, (probs, preds, labels) in enumerate(batches):
        for i in np.nonzero(np.asarray(preds) != np.asarray(labels))[0]:
            if len(out) >= max_failures:
                return out
            order = np.argsort(-np.asarray(probs[i]), kind="stable")[:3]
            out.append({"batch_idx": batch_idx, "sample_idx": int(i), "true_label": int(labels[i]), "predicted": int(preds[i]),
                        "confidence": float(probs[i][preds[i]]), "true_prob": float(probs[i][labels[i]]), "top3_preds": [int(j) for j in order],
                        "top3_probs": [float(probs[i][j]) for j in order]})
    return out


def train_evaluate(batches):
    """evaluate (ml/train.py:157-190) with nn.CrossEntropyLoss(): batches = [(logits f32 [b,10], labels [b]), ...] ->
    (mean of the per-batch mean nll, accuracy, per-class accuracy)."""
    total_loss, correct, total = 0.0, 0, 0
    cls_ok, cls_n = [0] * 10, [0] * 10
    for logits, labels in batches:
        r = per_cell(logits, labels)
        total_loss += float(r["nll"].mean())
        for p, t in zip(r["pred"], np.asarray(labels)):
            cls_n[t] += 1
            cls_ok[t] += int(p == t)
            correct += int(p == t)
            total += 1
    return total_loss / len(batches), correct / total, {i: cls_ok[i] / cls_n[i] if cls_n[i] > 0 else 0 for i in range(10)}


def aggregates(pred, conf, labels, n_bins, finite=None, edges=None):
    """sv_eval_stats in Python integers (the keys of Context.eval_stats_dict) from per-cell values: pred [B], conf f32 [B], labels [B],
    finite bool [B] (default: all).  The confidence sums are sums of int(conf * 2^30); the bins are ml/evaluate_v2.py:163 on float(conf)."""
    pred, labels = np.asarray(pred).astype(np.int64), np.asarray(labels).astype(np.int64)
    conf = np.asarray(conf, np.float32)
    finite = np.ones(len(pred), bool) if finite is None else np.asarray(finite, bool)
    edges = np.linspace(0, 1, n_bins + 1) if edges is None else np.asarray(edges, np.float64)
    out = {"confusion": [[0] * 10 for _ in range(10)], "n": 0, "n_correct": 0, "n_wrong": 0, "bad_labels": 0, "nonfinite": 0,
           "bin_count": [0] * n_bins, "bin_correct": [0] * n_bins, "bin_conf": [0] * n_bins, "tot_count": [0] * 3, "tot_correct": [0] * 3, "tot_conf": [0] * 3}
    for i in range(len(pred)):
        if not finite[i]:
            out["nonfinite"] += 1
            continue
        if not 0 <= labels[i] <= 9:
            out["bad_labels"] += 1
            continue
        ok = bool(pred[i] == labels[i])
        c = float(conf[i])
        fx = int(c * CONF_ONE)
        out["confusion"][labels[i]][pred[i]] += 1
        out["n"] += 1
        out["n_correct" if ok else "n_wrong"] += 1
        for k in (0, 1 if ok else 2):
            out["tot_count"][k] += 1
            out["tot_correct"][k] += int(ok)
            out["tot_conf"][k] += fx
        for b in range(n_bins):
            if c > edges[b] and c <= edges[b + 1]:
                out["bin_count"][b] += 1
                out["bin_correct"][b] += int(ok)
                out["bin_conf"][b] += fx
    return out


def per_cell_prob(probs, labels):
    """Probability-input mode (compute_calibration's argument, ml/evaluate_v2.py:152-154; the sv_eval_metrics comment): probs f32 [B,10],
    labels int [B] in 0..9 -> dict: pred (np.argmax of the f32 rows: first maximum, a NaN counting as the largest), conf and true_prob
    (the f32 input entries themselves), nll (-log in float64 of true_prob: +inf at 0, NaN below 0), correct, finite (all ten entries
    finite and 0 <= max <= 1)."""
    p = np.asarray(probs, np.float32)
    labels = np.asarray(labels).astype(np.int64)
    rows = np.arange(len(p))
    pred = np.argmax(p, 1)
    conf, true_prob = p[rows, pred], p[rows, labels]
    with np.errstate(divide="ignore", invalid="ignore"):
        nll = -np.log(true_prob.astype(np.float64))
        top = p.max(1)
        finite = np.isfinite(p).all(1) & (top >= 0) & (top <= 1)
    return {"pred": pred, "conf": conf, "true_prob": true_prob, "nll": nll, "correct": pred == labels, "finite": finite}


def aggregates_fast(pred, conf, labels, n_bins, finite=None, edges=None):
    """aggregates' vectorised twin for the large size: the same dictionary from np.searchsorted (the first edge >= conf, so bin k - 1 when
    1 <= k <= n_bins) and np.bincount.  tests/test_eval_ref.py holds it to aggregates for every entry of EDGE_SETS."""
    pred, labels = np.asarray(pred).astype(np.int64), np.asarray(labels).astype(np.int64)
    conf = np.asarray(conf, np.float32)
    finite = np.ones(len(pred), bool) if finite is None else np.asarray(finite, bool)
    edges = np.linspace(0, 1, n_bins + 1) if edges is None else np.asarray(edges, np.float64)
    bad = finite & ((labels < 0) | (labels > 9))
    valid = finite & ~bad
    pred, labels, c = pred[valid], labels[valid], conf[valid].astype(np.float64)
    ok = pred == labels
    fx = (c * CONF_ONE).astype(np.int64)                                   # towards zero, as int() of a float; the sums stay below 2^62
    k = np.searchsorted(edges, c, side="left")
    binned = (k >= 1) & (k <= n_bins)
    b = k[binned] - 1

    def per_bin(weights):
        out = np.zeros(n_bins, np.int64)
        np.add.at(out, b, weights[binned])
        return [int(v) for v in out]

    groups = (np.ones(len(ok), bool), ok, ~ok)
    return {"confusion": np.bincount(labels * 10 + pred, minlength=100).reshape(10, 10).tolist(), "n": int(valid.sum()), "n_correct": int(ok.sum()),
            "n_wrong": int((~ok).sum()), "bad_labels": int(bad.sum()), "nonfinite": int((~finite).sum()),
            "bin_count": per_bin(np.ones(len(ok), np.int64)), "bin_correct": per_bin(ok.astype(np.int64)), "bin_conf": per_bin(fx),
            "tot_count": [int(g.sum()) for g in groups], "tot_correct": [int((g & ok).sum()) for g in groups], "tot_conf": [int(fx[g].sum()) for g in groups]}


def ece_of(agg):
    """The expected calibration error of an aggregates() / eval_stats_dict dictionary, in float64 (ml/evaluate_v2.py:171-173)."""
    total = 0.0
    for count, good, fx in zip(agg["bin_count"], agg["bin_correct"], agg["bin_conf"]):
        if count:
            total += abs(good / count - fx / CONF_ONE / count) * count / agg["n"]
    return total


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
_POOL = {}


def random_cells(scale):
    """(logits f32 [SIZES[-1],10] at `scale`, labels int64): labels are the prediction for about 70 % of the cells, uniform otherwise.
    Every batch size takes a prefix.  Made once per scale and not writable."""
    if scale not in _POOL:
        rs = np.random.RandomState(2100 + int(scale))
        n = SIZES[-1]
        z = (rs.randn(n, 10) * scale).astype(np.float32)
        labels = np.where(rs.rand(n) < 0.7, z.argmax(1), rs.randint(0, 10, n)).astype(np.int64)
        z.setflags(write=False)
        labels.setflags(write=False)
        _POOL[scale] = (z, labels)
    return _POOL[scale]


def _row(hot, low=-1000.0):
    r = np.full(10, low, np.float32)
    r[list(hot)] = 0.0
    return r


def crafted_cells():
    """16 cells whose f32 softmax is known exactly (exp(-1000) is 0.0): 8 one-hot (conf 1.0), 4 two-way ties (0.5), 4 four-way ties
    (0.25); the prediction of a tie is its lowest class.  -> logits, labels, and what is known by hand: conf, pred."""
    hot = [(j,) for j in (0, 1, 2, 3, 5, 7, 8, 9)] + [(2, 6), (0, 9), (4, 5), (7, 8)] + [(1, 3, 5, 7), (0, 2, 4, 6), (6, 7, 8, 9), (3, 4, 8, 9)]
    z = np.stack([_row(h) for h in hot])
    pred = np.array([min(h) for h in hot])
    conf = np.array([1.0 / len(h) for h in hot], np.float32)
    labels = pred.copy()
    labels[[1, 6]] = [4, 0]                  # one-hot: 6 of 8 correct
    labels[[9, 10, 11]] = [9, 5, 8]          # two-way: 1 of 4 correct (the labels are the tie's other class: true_prob 0.5)
    labels[[12, 13, 15]] = [3, 9, 9]         # four-way: 1 of 4 correct
    return z, labels.astype(np.int64), conf, pred


ALL_EQUAL = np.zeros(10, np.float32)          # conf should be f32(0.1) > 0.1: bin 1 of 10 -- if 1 / den rounds as expected; the tests do not assume it


def failure_cells():
    """300 cells, 40 of them wrong, at the first and the last index and on both sides of the 256-cell workgroup boundary; every cell's
    ten logits are distinct (a permutation of ten spaced values), so the top-3 is unambiguous -- but for cell 255, whose second and
    third classes tie.  -> logits, labels int64, the wrong indices in order."""
    rs = np.random.RandomState(77)
    base = np.array([4.0, 2.5, 1.0, 0.0, -0.75, -1.5, -2.25, -3.0, -4.0, -5.5], np.float32)
    z = np.stack([base[rs.permutation(10)] + np.float32(0.01) * i for i in range(300)]).astype(np.float32)
    labels = z.argmax(1).astype(np.int64)
    keep = [0, 1, 254, 255, 256, 257, 299]
    wrong = sorted(keep + [int(i) for i in rs.permutation(np.arange(2, 298)) if i not in keep][:40 - len(keep)])
    for w in wrong:
        labels[w] = (labels[w] + 1 + w % 8) % 10                           # any class but the prediction
    tie = z[255].copy()
    order = np.argsort(-tie)
    tie[order[1]] = tie[order[2]]                                          # two classes now share the second place
    z[255] = tie
    if labels[255] == z[255].argmax():
        labels[255] = (labels[255] + 1) % 10
    return z, labels, np.array(wrong)


def edge_cells():
    """Cells for the edge tests.  -> dict of (logits, labels) pairs."""
    rs = np.random.RandomState(5)
    z = (rs.randn(90, 10) * 2).astype(np.float32)
    pred = z.argmax(1)
    out = {}
    z7 = z.copy()
    z7[:, 7] = -50.0                                                        # class 7 is never predicted ...
    lab = z7.argmax(1)
    lab[::3] = (lab[::3] + 1) % 10
    lab[lab == 7] = 6                                                       # ... and never a label: no support
    out["no_support"] = (z7, lab.astype(np.int64))
    out["all_correct"] = (z, pred.astype(np.int64))
    out["all_wrong"] = (z, ((pred + 3) % 10).astype(np.int64))
    lab = np.where(np.arange(90) % 4 == 0, (pred + 1) % 10, pred).astype(np.int64)
    bad = lab.copy()
    bad[10], bad[80] = 10, -1
    out["bad_labels"] = (z, bad)
    zn = z.copy()
    zn[5, 3] = np.nan
    zn[70, 0] = np.inf
    out["nonfinite"] = (zn, lab)
    out["mixed"] = (z, lab)
    return out


# ---- inputs of tests/test_gpu_eval_modes.py: probability mode, caller bin edges, the long failure list -------------------------------------
EDGE_SETS = {                                  # name -> (bin_edges as doubles, n_bins)
    "uniform10": (np.linspace(0, 1, 11), 10),                               # the default
    "decimal": (np.array([0, 0.1, 0.3, 0.7, 1.0]), 4),                      # f32(0.1), f32(0.3) lie above their double edge, f32(0.7) below
    "repeated": (np.array([0, 0.5, 0.5, 0.5, 1.0]), 4),                     # bins 1 and 2 are empty whatever the cells
    "inner": (np.array([0.2, 0.4, 0.9]), 2),                                # cells below 0.2 and above 0.9 are in no bin
    "one": (np.array([0.125, 1.0]), 1),                                     # a conf of 0.125 sits on the open lower edge: no bin
    "fine64": (np.linspace(0, 1, 65) ** 2, 64),                             # 65 non-uniform edges: all of the LDS copy
}


def _prob_row(top, at, rest):
    r = np.full(10, rest, np.float32)
    r[at] = top
    return r


def prob_cells():
    """Rows for the probability-input mode -> (probs f32 [N,10], labels int64 [N], marks: name -> row index).  The first 2 * 257 rows are
    the torch-CPU f32 softmax of the first 257 random_cells at scale 1 and at scale 30 (many rows with conf == 1.0, entries that are
    denormal or zero), with their labels.  Then the crafted rows, each named in marks for what it is there for:
      tiny          all ten 1e-12: valid, the fixed-point term is 0, bin 0 of uniform edges
      zeros         all ten 0: pred 0, counted in n, in no bin of edges that start at 0; label 0: true_prob 0, nll +inf
      sub_unit      all ten 0.75 * 2^-30: the fixed-point term truncates to 0 (rounding would give 1)
      small         top f32(0.001): 0.001 * 2^30 is no integer, the term truncates
      negatives     top 0.6, the others between -3 and -1, a wrong cell: its top-3 is 0.6, then two entries of -1.0, lowest class first
      neg_label     a valid wrong cell whose label points at -0.05: true_prob < 0, nll NaN
      above_one     top nextafter(1, 2): not finite by the mode's rule;  neg_top: top -0.25, all others lower: the same
      nan, inf      one NaN entry (class 3, not the first: np.argmax gives 3), one +inf entry: not finite
      on_0.1, on_0.3, on_0.7, on_0.125, below_0.5   the maximum is exactly f32(0.1), f32(0.3), f32(0.7), 0.125, nextafter(f32(0.5), 0)
    Made once, not writable."""
    if "prob" not in _POOL:
        import torch
        parts, labels = [], []
        for scale in SCALES:
            z, lab = random_cells(scale)
            parts.append(torch.softmax(torch.from_numpy(z[:257].copy()), 1).numpy())
            labels.append(lab[:257])
        f = np.float32
        crafted = [
            ("tiny", _prob_row(1e-12, 0, 1e-12), 0),
            ("zeros", np.zeros(10, f), 0),
            ("sub_unit", _prob_row(0.75 * 2.0 ** -30, 0, 0.75 * 2.0 ** -30), 4),
            ("small", _prob_row(0.001, 6, 0.0005), 6),
            ("negatives", np.array([-2.5, -1.0, -3.0, -1.5, 0.6, -1.0, -2.0, -1.25, -2.75, -1.75], f), 7),
            ("neg_label", np.array([0.9, 0.05, -0.05, 0.1, 0, 0, 0, 0, 0, 0], f), 2),
            ("above_one", _prob_row(np.nextafter(f(1), f(2)), 2, 0.0), 2),
            ("neg_top", _prob_row(-0.25, 5, -0.5), 5),
            ("nan", np.array([0.1, 0.2, 0.05, np.nan, 0.3, 0.05, 0.1, 0.1, 0.05, 0.05], f), 4),
            ("inf", np.array([0.1, 0.2, 0.05, 0.05, 0.3, 0.05, np.inf, 0.1, 0.05, 0.05], f), 6),
            ("on_0.1", _prob_row(f(0.1), 9, 0.05), 9),
            ("on_0.3", _prob_row(f(0.3), 1, 0.07), 0),
            ("on_0.7", _prob_row(f(0.7), 8, 0.03), 8),
            ("on_0.125", _prob_row(0.125, 3, 0.0625), 3),
            ("below_0.5", _prob_row(np.nextafter(f(0.5), f(0)), 7, 0.05), 2),
        ]
        at = 2 * 257
        marks = {name: at + i for i, (name, _, _) in enumerate(crafted)}
        probs = np.concatenate(parts + [np.stack([r for _, r, _ in crafted])]).astype(np.float32)
        lab = np.concatenate(labels + [np.array([c for _, _, c in crafted], np.int64)])
        probs.setflags(write=False)
        lab.setflags(write=False)
        _POOL["prob"] = (probs, lab, marks)
    return _POOL["prob"]


LONG_TILE = 300                                # the all-wrong tile: cells 76,800 .. 77,055, past the seam between scan chunks at tile 256
LONG_SEAMS = (0, 255, 256, 65535, 65536, 65791, 131071, 131072, 262143, 262144, 262145)


def long_list_cells():
    """The SIZES[-1] = 262,146 random_cells(1.0) with each label set to the row's argmax, but for 300 wrong cells: LONG_SEAMS (the ends of
    tile 0; both sides of cell 65,536, where k_eval_scan goes from its first chunk of 256 tiles to the second, and the end of that
    chunk's first tile; both sides of 131,072; the last cell of a workgroup's first tile, 262,143, and the two cells of workgroup 0's
    second tile), cell 100 (tile 0 then holds another count of wrong cells than tile 1,024, the tile whose count a workgroup-indexed write
    would put in its place), all 256 cells of tile LONG_TILE, and 32 more drawn from the whole range.
    -> logits f32, labels int64, the wrong indices in order.  Made once, not writable."""
    if "long" not in _POOL:
        z, _ = random_cells(1.0)
        n = len(z)
        pred = z.argmax(1).astype(np.int64)
        fixed = set(LONG_SEAMS) | {100} | set(range(LONG_TILE * 256, LONG_TILE * 256 + 256))
        rs = np.random.RandomState(2121)
        extra = [int(i) for i in rs.permutation(n) if int(i) not in fixed][:300 - len(fixed)]
        wrong = np.array(sorted(fixed | set(extra)), np.int64)
        labels = pred.copy()
        labels[wrong] = (pred[wrong] + 1 + wrong % 8) % 10                  # any class but the prediction
        labels.setflags(write=False)
        wrong.setflags(write=False)
        _POOL["long"] = (z, labels, wrong)
    return _POOL["long"]
