"""Writes tests/golden/eval_goldens.npz: what the REFERENCE's own ml/evaluate_v2.py (evaluate_dataset, compute_calibration,
find_failures) and ml/train.py (evaluate) return, on torch CPU, for the reference's DigitCNNv3 with the seeded weights of
tests/golden/model_v3_se.npz and a 3-batch loader (sizes 5, 5 and 3) of that file's first 13 inputs.  The labels are the reference's own
predictions but for three cells: the last of batch 0, the first of batch 1 (the two sides of a batch boundary) and the last of batch 2.
Results only; the weights and inputs are regenerated from their seeds.

Run where the reference tree is available:   python tests/golden/make_eval_goldens.py [reference root, default /root/reference]"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import model_v3_ref  # noqa: E402

DEFAULT_ROOT = "/root/reference"
BATCHES = (5, 5, 3)
WRONG = (4, 5, 12)


def reference_modules(ref_root):
    """The reference's ml/evaluate_v2.py, ml/train.py (None when its own imports cannot be met) and ml/model_v3.py as modules.  Both
    scripts import torchvision at the top for their command lines only: where it is not installed an empty stand-in takes its place for
    the import.  The drop-in modules of this repository have the same names, so the reference's directory goes first on sys.path and any
    module of those names loaded before is set aside for the duration."""
    ml = os.path.join(ref_root, "ml")
    if not os.path.exists(os.path.join(ml, "evaluate_v2.py")):
        raise FileNotFoundError(ml)
    names = ("evaluate_v2", "train", "model", "model_v3", "datasets")
    saved = {n: sys.modules.pop(n) for n in names if n in sys.modules}
    stub = None
    try:
        importlib.import_module("torchvision")
    except ImportError:
        stub = types.ModuleType("torchvision")
        stub.datasets, stub.transforms = types.ModuleType("torchvision.datasets"), types.ModuleType("torchvision.transforms")
        sys.modules.update({"torchvision": stub, "torchvision.datasets": stub.datasets, "torchvision.transforms": stub.transforms})
    sys.path.insert(0, ml)
    try:
        ev = importlib.import_module("evaluate_v2")
        m3 = importlib.import_module("model_v3")
        try:
            tr = importlib.import_module("train")
        except Exception:
            tr = None
    finally:
        sys.path.remove(ml)
        for n in names:
            sys.modules.pop(n, None)
        sys.modules.update(saved)
        if stub is not None:
            for n in ("torchvision", "torchvision.datasets", "torchvision.transforms"):
                sys.modules.pop(n, None)
    return ev, tr, m3


def reference_model(m3, w_seed):
    torch.manual_seed(0)
    model = m3.DigitCNNv3(use_se=True)
    full = model.state_dict()
    sd = model_v3_ref.random_state_dict_v3(w_seed, True)
    model.load_state_dict({**{k: v for k, v in full.items() if k.endswith("num_batches_tracked")}, **sd}, strict=True)
    return model.eval()


def loader_of(x, labels):
    at = np.concatenate([[0], np.cumsum(BATCHES)])
    return [(torch.from_numpy(x[a:b].copy()), torch.from_numpy(labels[a:b].copy())) for a, b in zip(at[:-1], at[1:])]


def inputs(golden):
    """The 13 cells and their labels from the model_v3_se.npz record: labels = argmax of the stored reference logits, WRONG moved on."""
    x = model_v3_ref.inputs(int(golden["x_seed"]), int(golden["n"]))[:sum(BATCHES)]
    labels = golden["logits"][:sum(BATCHES)].argmax(1).astype(np.int64)
    for i in WRONG:
        labels[i] = (labels[i] + 1 + i % 7) % 10
    return x, labels


def plain(d):
    """A result dictionary without its arrays, JSON-ready (numpy scalars to Python, integer keys to strings)."""
    if isinstance(d, dict):
        return {str(k): plain(v) for k, v in d.items() if not isinstance(v, np.ndarray)}
    if isinstance(d, (list, tuple)):
        return [plain(v) for v in d]
    return d.item() if isinstance(d, np.generic) else d


def main(ref_root):
    ev, tr, m3 = reference_modules(ref_root)
    golden = np.load(os.path.join(HERE, "model_v3_se.npz"))
    model = reference_model(m3, int(golden["w_seed"]))
    x, labels = inputs(golden)
    loader = loader_of(x, labels)
    cpu = torch.device("cpu")
    res = ev.evaluate_dataset(model, loader, cpu, "golden")
    out = {"dataset": json.dumps(plain(res)), "predictions": res["predictions"], "labels": res["labels"], "probabilities": res["probabilities"],
           "calibration15": json.dumps(plain(ev.compute_calibration(res["probabilities"], res["labels"], 15)))}
    for m in (2, 100):
        fails = ev.find_failures(model, loader, cpu, m)
        out[f"failures{m}"] = json.dumps([plain({k: v for k, v in f.items() if k != "image"}) for f in fails])
    criterion = torch.nn.CrossEntropyLoss()
    if tr is not None:
        loss, acc, per_class = tr.evaluate(model, loader, criterion, cpu)
        source = "ml/train.py evaluate"
    else:
        # train.py's own imports (its datasets module) cannot be met here: the three results of its loop (:171-190) from torch's criterion on
        # the reference model's logits and from the predictions evaluate_dataset returned
        with torch.no_grad():
            loss = sum(criterion(model(d), t).item() for d, t in loader) / len(loader)
        ok = res["predictions"] == res["labels"]
        acc = float(ok.mean())
        per_class = {i: float(ok[res["labels"] == i].mean()) if (res["labels"] == i).any() else 0 for i in range(10)}
        source = "torch.nn.CrossEntropyLoss on the reference model's logits"
    out["evaluate"] = json.dumps({"loss": float(loss), "accuracy": float(acc), "per_class_acc": {str(k): float(v) for k, v in per_class.items()}, "source": source})
    np.savez_compressed(os.path.join(HERE, "eval_goldens.npz"), **out)
    print({k: (v if isinstance(v, str) else v.shape) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_ROOT)
