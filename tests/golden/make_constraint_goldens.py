"""Writes tests/golden/constraint_goldens.npz: what the REFERENCE's own pipeline/constraint_resolver.py ConstraintResolver (imported
from the reference tree) returns for the generated frames and the crafted cases of tests/constraint_ref.py.  Seeds and outputs only:
the inputs are regenerated from the seeds.

The reference is also run subclassed so that its hidden singles come back sorted instead of in set order; `order_differs` records per
frame whether the outcome then differs (any field, with `resolved` compared as the set of placements: the order of cells_resolved
follows the order of the hidden singles on every frame, `resolved_differs`) and `valid_differs` whether is_valid does.  The coverage conditions below are checked here, on
the reference's results alone.

Run where the reference tree is available:   python tests/golden/make_constraint_goldens.py [reference root, default /root/reference]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import constraint_ref as cr  # noqa: E402


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "pipeline"))
    import constraint_resolver as ref

    seen = {"distinct": 0}

    class Probe(ref.ConstraintResolver):
        def find_hidden_singles(self):
            out = super().find_hidden_singles()
            seen["distinct"] = max(seen["distinct"], len(out))
            return out

    class Sorted(ref.ConstraintResolver):
        def find_hidden_singles(self):
            return sorted(super().find_hidden_singles())

    def arrays(res):
        cand = np.array([sum(1 << d for d in c.candidates) for c in res.cells], np.uint16)
        resolved = np.full((81, 2), cr.NONE, np.uint8)
        for i, (r, c, v) in enumerate(res.cells_resolved):
            resolved[i] = (9 * r + c, v)
        assert [c.value for c in res.cells] == [v for row in res.grid for v in row]
        cc = res.contradiction_cell
        return {"grid": np.array(res.grid, np.uint8).reshape(81), "candidates": cand, "is_valid": np.uint8(res.is_valid),
                "iterations": np.int32(res.iterations), "contradiction_cell": np.uint8(cr.NONE if cc is None else 9 * cc[0] + cc[1]),
                "n_resolved": np.uint8(len(res.cells_resolved)), "resolved": resolved,
                "is_fixed": np.array([c.is_fixed for c in res.cells], np.uint8)}

    def run(digits, conf, max_iterations):
        out = {key: [] for key in cr.FIELDS + ("order_differs", "resolved_differs", "valid_differs", "distinct")}
        for f in range(digits.shape[0]):
            grid = [[int(v) for v in row] for row in digits[f].reshape(9, 9)]
            c = None if conf is None else [[float(v) for v in row] for row in conf[f].reshape(9, 9)]
            seen["distinct"] = 0
            real = arrays(Probe(grid, c).propagate(max_iterations))
            alt = arrays(Sorted(grid, c).propagate(max_iterations))
            for key in cr.FIELDS:
                out[key].append(real[key])
            for res in (real, alt):                     # the outcome: `resolved` as what was placed, not in which order
                res["placed"] = np.sort(res["resolved"].astype(np.int32) @ np.array([16, 1]))
            out["order_differs"].append(np.uint8(any(real[key].tobytes() != alt[key].tobytes() for key in cr.FIELDS + ("placed",) if key != "resolved")))
            out["resolved_differs"].append(np.uint8(real["resolved"].tobytes() != alt["resolved"].tobytes()))
            out["valid_differs"].append(np.uint8(real["is_valid"] != alt["is_valid"]))
            out["distinct"].append(np.int32(seen["distinct"]))
        return {key: np.stack(v) for key, v in out.items()}

    save = {"seed": cr.GOLDEN_SEED, "per_kind": cr.PER_KIND}
    digits, conf = cr.frames()
    gen = run(digits, conf, 100)
    for key, v in gen.items():
        save[f"gen.{key}"] = v
    n = cr.PER_KIND
    for k, kind in enumerate(cr.KINDS):
        rows = slice(k * n, (k + 1) * n)
        print(f"{kind}: outcomes disagree in {int(gen['order_differs'][rows].sum())} / {n}, cells_resolved in {int(gen['resolved_differs'][rows].sum())}, is_valid disagrees in {int(gen['valid_differs'][rows].sum())}, "
              f"invalid {int((gen['is_valid'][rows] == 0).sum())}, iterations up to {int(gen['iterations'][rows].max())}")
    top = int(gen["distinct"].max())
    print(f"distinct hidden entries in one pass: at most {top}; tables of 32 slots (>= 5 entries) in {int((gen['distinct'] >= 5).sum())} frames, "
          f"of 128 (>= 19) in {int((gen['distinct'] >= 19).sum())}, of 512 (>= 77) in {int((gen['distinct'] >= 77).sum())}")
    assert gen["order_differs"].sum() >= 25, "too few frames where set order and sorted order disagree"
    assert gen["valid_differs"].sum() >= 3, "too few frames where is_valid depends on the order"
    assert gen["order_differs"][:n].sum() == 0, "a consistent frame depends on the order"
    assert top >= 19, "no frame grows the table to 128 slots"
    for name, (cd, cc, it) in cr.crafted_cases().items():
        for key, v in run(cd, cc, it).items():
            save[f"case.{name}.{key}"] = v
    path = os.path.join(HERE, "constraint_goldens.npz")
    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
