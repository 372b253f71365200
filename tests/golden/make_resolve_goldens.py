"""Writes tests/golden/resolve_goldens.npz: what the REFERENCE's own pipeline/validator.py validate_predictions and
pipeline/conflict_resolver.py resolve_conflicts (imported from the reference tree) return for the generated frames, the crafted cases
and the argument variants of tests/resolve_ref.py.  Seeds and outputs only: the inputs are regenerated from the seeds.  The real-probability frames (`real.*`, `real_k2.*`, `real_k4.*`)
and the threshold variants (`real_minalt.<m>.*`, run through ConflictResolver(min_alternative_confidence=m)) also store a digest of
their inputs, so a platform whose exp() rounds a probability the other way is told apart from a wrong restatement.  Keys are only
ever added: the script refuses to write a file in which a key of the existing one is missing or has other bytes.

The coverage figures (`stats`) come from the reference too: its ConflictResolver is subclassed only to count the candidates of a path
before its cut to 10, and heapq.nsmallest is wrapped only to see how many invalid paths a depth produced.

Run where the reference tree is available:   python tests/golden/make_resolve_goldens.py [reference root, default /root/reference]"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resolve_ref as rr  # noqa: E402


def input_digest(index, prob):
    return hashlib.sha256(np.ascontiguousarray(index).tobytes() + np.ascontiguousarray(prob).tobytes()).hexdigest()


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "pipeline"))
    import conflict_resolver as cr
    from validator import CellInfo, validate_predictions

    seen = {"cand": 0, "invalid": 0, "empty": 0}

    class Probe(cr.ConflictResolver):
        def _get_correction_candidates(self, cells):
            v = validate_predictions(cells)
            seen["cand"] = max(seen["cand"], sum(1 for c in cells if (c.row, c.col) in v.cells_in_conflict for d, p in c.alternatives
                                                 if d != c.digit and p >= self.min_alternative_confidence))
            return super()._get_correction_candidates(cells)

    real_nsmallest = cr.heapq.nsmallest

    def nsmallest(n, paths):
        paths = list(paths)
        seen["invalid"] = max(seen["invalid"], len(paths))
        seen["empty"] |= not paths
        return real_nsmallest(n, paths)

    cr.ConflictResolver = Probe
    cr.heapq.nsmallest = nsmallest

    def run(index, prob, beam_width, max_corrections, min_alt=None):
        n, _, k = index.shape
        out = {key: [] for key in rr.FIELDS + ("stats", "descriptions")}
        for f in range(n):
            cells = [CellInfo(row=x // 9, col=x % 9, digit=int(index[f, x, 0]), confidence=float(prob[f, x, 0]),
                              alternatives=[(int(index[f, x, j]), float(prob[f, x, j])) for j in range(1, k)]) for x in range(81)]
            first = validate_predictions(cells)
            seen.update(cand=0, invalid=0, empty=0)
            if min_alt is None:
                res = cr.resolve_conflicts(cells, beam_width=beam_width, max_corrections=max_corrections)
            else:
                res = cr.ConflictResolver(beam_width=beam_width, max_corrections=max_corrections, min_alternative_confidence=min_alt).resolve(cells)
            oi = np.full((81, k), rr.PAD_INDEX, np.uint8)
            op = np.full((81, k), rr.PAD_PROB, np.float32)
            for c in res.cells:
                x = 9 * c.row + c.col
                oi[x, 0], op[x, 0] = c.digit, c.confidence
                for j, (d, p) in enumerate(c.alternatives):
                    oi[x, 1 + j], op[x, 1 + j] = d, p
            assert [[int(oi[9 * r + c, 0]) for c in range(9)] for r in range(9)] == res.grid
            count = np.zeros(81, np.uint8)
            for conflict in res.validation_result.conflicts:
                for r, c in conflict.cells:
                    count[9 * r + c] += 1
            cc = np.zeros((3, 3), np.uint8)
            cf = np.zeros((3, 2), np.float32)
            for i, m in enumerate(res.corrections_made):
                cc[i] = (9 * m.row + m.col, m.original_digit, m.new_digit)
                cf[i] = (m.original_confidence, m.alternative_confidence)
            vals = {"digits": oi[:, 0].copy(), "conf": op[:, 0].copy(), "index": oi, "prob": op, "success": np.uint8(res.success),
                    "num_conflicts_before": np.int32(first.num_conflicts), "num_conflicts_after": np.int32(res.validation_result.num_conflicts),
                    "conflict_count": count, "n_corrections": np.uint8(len(res.corrections_made)), "corr_cells": cc, "corr_conf": cf,
                    "paths_explored": np.int32(res.paths_explored), "score": np.float64(res.score),
                    "stats": np.array((len(res.corrections_made) if res.success else 0, seen["empty"], seen["cand"], seen["invalid"]), np.int32),
                    "descriptions": "|".join(c.description for c in first.conflicts) + "||" + "|".join(c.description for c in res.validation_result.conflicts)}
            for key, v in vals.items():
                out[key].append(v)
        return {key: np.stack(v) if key != "descriptions" else np.array(v) for key, v in out.items()}

    save = {"seed": rr.GOLDEN_SEED, "n": rr.GOLDEN_N}
    index, prob = rr.frames(rr.GOLDEN_SEED, rr.GOLDEN_N)
    for key, v in run(index, prob, 5, 3).items():
        save[f"gen.{key}"] = v
    s = save["gen.stats"]
    print("valid on entry", int((save["gen.num_conflicts_before"] == 0).sum()), "success at depth 1/2/3", [int((s[:, 0] == d).sum()) for d in (1, 2, 3)],
          "failed with a beam", int(((save["gen.success"] == 0) & (s[:, 1] == 0)).sum()), "empty beam", int(s[:, 1].sum()),
          ">10 candidates", int((s[:, 2] > 10).sum()), ">5 invalid paths", int((s[:, 3] > 5).sum()))
    for name, (ci, cp) in rr.crafted_cases().items():
        for key, v in run(ci, cp, 5, 3).items():
            save[f"case.{name}.{key}"] = v
    for name, (seed, n, k, beam, maxc) in rr.VARIANTS.items():
        vi, vp = rr.frames(seed, n, k)
        for key, v in run(vi, vp, beam, maxc).items():
            save[f"var.{name}.{key}"] = v
    real = {"real": (rr.REAL_SEED, rr.REAL_N, 3), **rr.REAL_VARIANTS}
    for name, (seed, n, k) in real.items():
        ri, rp = rr.real_frames(seed, n, k)
        save[f"{name}.input_sha256"] = input_digest(ri, rp)
        for key, v in run(ri, rp, 5, 3).items():
            save[f"{name}.{key}"] = v
        s = save[f"{name}.stats"]
        print(name, "valid on entry", int((save[f"{name}.num_conflicts_before"] == 0).sum()), "success at depth 1/2/3",
              [int((s[:, 0] == d).sum()) for d in (1, 2, 3)], "failed", int((save[f"{name}.success"] == 0).sum()),
              ">10 candidates", int((s[:, 2] > 10).sum()), ">5 invalid paths", int((s[:, 3] > 5).sum()))
    for m in rr.MINALT:
        mi, mp, exact, above = rr.minalt_frames(m)
        save[f"{rr.minalt_name(m)}.input_sha256"] = input_digest(mi, mp)
        for key, v in run(mi, mp, 5, 3, min_alt=m).items():
            save[f"{rr.minalt_name(m)}.{key}"] = v
        print(rr.minalt_name(m), "alternative == f32(m): success", save[f"{rr.minalt_name(m)}.success"][exact].tolist(),
              "one ulp above:", save[f"{rr.minalt_name(m)}.success"][above].tolist())
    path = os.path.join(HERE, "resolve_goldens.npz")
    if os.path.exists(path):
        with np.load(path) as old:
            for key in old.files:
                new = np.asarray(save[key])
                assert new.dtype == old[key].dtype and new.shape == old[key].shape and new.tobytes() == old[key].tobytes(), f"{key} would change"
            print(len(old.files), "existing keys keep their bytes;", len(save) - len(old.files), "added")
    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
