"""MI355X drop-in for the reference's ml/evaluate_v2.py (and ml/train.py's `evaluate`): the same functions, arguments and result keys.
The model's forward is the existing HIP forward (DigitCNN, DigitCNNv3, DigitCNNv3Light); what the reference then does on the host, one
cell, class and bin at a time -- softmax, argmax, confusion counts, reliability bins, the failure list -- is one pass of K21
(csrc/k21_eval.hip, Context.eval_metrics) over the logits where they are, accumulated across the loader's batches in one device block.
Only that block, and the arrays the reference's dictionary itself carries, come to the host.

The plot and print helpers of the reference need matplotlib and are not here.  GPU only; there is no CPU fallback."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bootstrap import package  # noqa: E402
sys.path.pop(0)
_rt = package().runtime

_ONE = float(_rt.Context.EVAL_CONF_ONE)


def _context(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("evaluate_v2 (MI355X): the metrics run on the GPU; there is no CPU fallback")
    return _rt.default_context(device)


def _mean(fixed_sum, count):
    """Mean confidence of `count` cells from their fixed-point sum; 0 for none, as the reference has it."""
    return fixed_sum / _ONE / count if count else 0


def _calibration(agg, n_bins):
    """compute_calibration's dictionary (reference ml/evaluate_v2.py:156-181) from the bins of an aggregate block."""
    edges = np.linspace(0, 1, n_bins + 1)
    out = {"bin_centers": [], "bin_accuracies": [], "bin_confidences": [], "bin_counts": []}
    for i in range(n_bins):
        count = agg["bin_count"][i]
        if count > 0:
            out["bin_centers"].append((edges[i] + edges[i + 1]) / 2)
            out["bin_accuracies"].append(np.float64(agg["bin_correct"][i] / count))
            out["bin_confidences"].append(np.float32(_mean(agg["bin_conf"][i], count)))
            out["bin_counts"].append(int(count))
    total = agg["n"]
    ece = 0
    for acc, conf, count in zip(out["bin_accuracies"], out["bin_confidences"], out["bin_counts"]):
        ece += abs(acc - conf) * count / total
    out["ece"] = float(ece)
    return out


def _per_class(confusion):
    """Per-class precision, recall, F1, support and accuracy (reference ml/evaluate_v2.py:104-125) from confusion[label][pred]; a class
    without support is left out."""
    cm = np.asarray(confusion, np.int64)
    out = {}
    for cls in range(10):
        support = int(cm[cls].sum())
        if support == 0:
            continue
        tp = int(cm[cls, cls])
        fp = int(cm[:, cls].sum()) - tp
        fn = support - tp
        precision = tp / (tp + fp) if (tp + fp) > 0 else 0
        recall = tp / (tp + fn) if (tp + fn) > 0 else 0
        f1 = 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0
        out[cls] = {"precision": float(precision), "recall": float(recall), "f1": float(f1), "support": support, "accuracy": float(tp / support)}
    return out


def _run(model, loader, device, want, max_failures=0, per_batch=None):
    """The model's forward and K21 over every batch of `loader`, accumulating into one stats block.  -> (aggregate dict, per-batch list of
    K21's output dicts -- with the batch's labels under "labels" --, batch sizes, the failure buffer or None).  per_batch(out, data):
    called after each batch's launch."""
    ctx = _context(device)
    model.eval()
    stats = ctx.eval_stats_buffer()
    outs, sizes, failures, seen = [], [], None, 0
    with torch.no_grad():
        for data, target in loader:
            data, target = data.to(ctx.device), target.to(ctx.device)
            logits = model(data)
            out, _ = ctx.eval_metrics(logits, target, want=want, stats=stats, accumulate=True, index_base=seen, max_failures=max_failures, failures=failures,
                                      read_back=False)
            failures = out.get("failures")
            out["labels"] = target
            if per_batch is not None:
                per_batch(out, data)
            outs.append(out)
            sizes.append(int(target.shape[0]))
            seen += sizes[-1]
    agg = _rt.Context.eval_stats_dict(stats, 10)          # the one read-back of the aggregates
    if agg["bad_labels"]:
        raise ValueError(f"{agg['bad_labels']} labels are outside 0..9")
    return agg, outs, sizes, failures


def evaluate_dataset(model: nn.Module, loader, device, dataset_name: str = "test") -> dict:
    """Evaluate `model` on a dataset: the reference's dictionary (ml/evaluate_v2.py:67-147), same keys and types."""
    agg, outs, _, _ = _run(model, loader, device, ("probs", "pred"))
    n, good, wrong = agg["tot_count"]
    cat = lambda key, dtype: (torch.cat([o[key] for o in outs]).cpu().numpy().astype(dtype) if outs else np.array([]))
    return {
        "dataset": dataset_name,
        "samples": int(n + agg["nonfinite"]),
        "accuracy": float(good / n) if n else float("nan"),
        "per_class": _per_class(agg["confusion"]),
        "mean_confidence": float(_mean(agg["tot_conf"][0], n)),
        "correct_confidence": float(_mean(agg["tot_conf"][1], good)),
        "incorrect_confidence": float(_mean(agg["tot_conf"][2], wrong)),
        "calibration": _calibration(agg, 10),
        "predictions": cat("pred", np.int64),
        "labels": cat("labels", np.int64),
        "probabilities": cat("probs", np.float32),
    }


def compute_calibration(probs: np.ndarray, labels: np.ndarray, n_bins: int = 10, device="cuda") -> dict:
    """Calibration metrics for a reliability diagram from given probabilities [N,10] and labels [N] (reference
    ml/evaluate_v2.py:150-181): K21 in its probability-input mode.  numpy arrays are uploaded; CUDA tensors are used where they are."""
    if isinstance(probs, torch.Tensor) and probs.is_cuda:
        device = probs.device
    ctx = _context(device)
    p = torch.as_tensor(probs).to(ctx.device, torch.float32)
    t = torch.as_tensor(labels).to(ctx.device)
    if t.dtype not in (torch.int64, torch.int32):
        t = t.to(torch.int64)
    _, agg = ctx.eval_metrics(p, t, n_bins=n_bins, want=(), probabilities=True)
    return _calibration(agg, n_bins)


def find_failures(model: nn.Module, loader, device, max_failures: int = 100) -> list:
    """Misclassified samples, the first max_failures in loader order (reference ml/evaluate_v2.py:184-220): the same record keys;
    batch_idx and sample_idx are rebuilt from the record's global index and the loader's batch sizes, image is the sample as the
    loader gave it."""
    if max_failures <= 0:
        return []
    batches = []
    agg, _, sizes, buf = _run(model, loader, device, (), max_failures=max_failures, per_batch=lambda out, data: batches.append(data))
    if buf is None:                                        # an empty loader
        return []
    records = _rt.Context.eval_failures(buf, min(max_failures, agg["n_wrong"]))
    starts = np.concatenate([[0], np.cumsum(sizes)])
    out = []
    for r in records:
        b = int(np.searchsorted(starts, r["index"], side="right") - 1)
        i = int(r["index"] - starts[b])
        out.append({"batch_idx": b, "sample_idx": i, "true_label": int(r["label"]), "predicted": int(r["pred"]), "confidence": float(r["conf"]),
                    "true_prob": float(r["true_prob"]), "top3_preds": r["top3_index"].tolist(), "top3_probs": r["top3_prob"].tolist(),
                    "image": batches[b][i].cpu().numpy()})
    return out


def evaluate(model: nn.Module, loader, criterion: nn.Module, device) -> tuple:
    """(loss, accuracy, per_class_acc) as the reference's ml/train.py:157-190 returns them: the loss is the mean over the batches of each
    batch's mean negative log-likelihood, summed in the loader's order.  Only nn.CrossEntropyLoss() with its default arguments is taken."""
    default = (isinstance(criterion, nn.CrossEntropyLoss) and criterion.weight is None and criterion.reduction == "mean" and criterion.ignore_index == -100
               and getattr(criterion, "label_smoothing", 0.0) == 0.0)
    if not default:
        raise NotImplementedError("evaluate (MI355X): only nn.CrossEntropyLoss() with default arguments is supported; K21 computes the plain "
                                  "negative log-likelihood of softmax(logits)")
    agg, outs, sizes, _ = _run(model, loader, device, ("nll",))
    total_loss = 0.0
    for loss in [o["nll"].mean() for o in outs]:          # a batch's mean on the device, one scalar each to the host
        total_loss += loss.item()
    cm = np.asarray(agg["confusion"], np.int64)
    per_class_acc = {i: int(cm[i, i]) / int(cm[i].sum()) if cm[i].sum() > 0 else 0 for i in range(10)}
    return total_loss / len(sizes), agg["n_correct"] / agg["n"], per_class_acc
