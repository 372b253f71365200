"""Plain-Python restatement of run_v2's validation and beam-search conflict repair (pipeline/validator.py:69-159,
pipeline/conflict_resolver.py:58-286 as pipeline/run_v2.py:344-371 calls them), arrays in, arrays out, and the seeded frame generator
the resolve tests share.  Written from the rules in DESIGN.md ("K9"), not from csrc/k9_resolve.hip: every path is a full copy of the
frame and is validated from nothing, which is exactly what the kernel avoids.

A frame is index u8 [81,k] and prob f32 [81,k] (sv_softmax_topk_f32's output): digit = index[.,0], confidence = prob[.,0], the
alternatives are slots 1..k-1.  Probabilities are held as Python floats (doubles) holding f32 values, as run_v2 holds them.

The score's claim ("exact to the bit") has a domain: every confidence that can enter a path's sum -- top-1 of a filled cell, any
eligible alternative -- is 0 or at least 2^-18; then the sum of up to 81 of them is exact in a double in any order, so CPython's sum()
(whose rounding changed in 3.12), math.fsum, a running sum and the kernel's reduction agree.  Softmax top-1 values (>= 0.1) and
alternatives that passed min_alt >= 2^-18 are inside it; `scored=` hands out the confidences of every scored path so a test can prove it.

`mutant=` (tests only) restates the resolver with one plausible float mistake of a kernel: "f32_sum" keeps the confidence sum in
np.float32, "f32_score" keeps the sum in double but computes the average and the final expression in np.float32, "f32_threshold"
tests eligibility as np.float32(p) >= np.float32(min_alt).
"""
import math

import numpy as np

ROWS = [[9 * r + c for c in range(9)] for r in range(9)]
COLS = [[9 * r + c for r in range(9)] for c in range(9)]
BOXES = [[9 * (3 * (b // 3) + i) + 3 * (b % 3) + j for i in range(3) for j in range(3)] for b in range(9)]
UNITS = ROWS + COLS + BOXES            # the order validate_predictions reports conflicts in

PAD_INDEX, PAD_PROB = 255, 0.0         # what an alternative slot holds when a correction left the cell with fewer alternatives


class Frame:
    """The 81 cells of one path: digit, confidence, and the list of (digit, prob) alternatives of every cell."""

    def __init__(self, digit, conf, alts):
        self.digit, self.conf, self.alts = digit, conf, alts

    @classmethod
    def from_arrays(cls, index, prob):
        k = index.shape[1]
        return cls([int(v) for v in index[:, 0]], [float(v) for v in prob[:, 0]],
                   [[(int(index[x, j]), float(prob[x, j])) for j in range(1, k)] for x in range(81)])

    def corrected(self, x, slot):
        """A copy with alternative `slot` of cell x installed: the old digit goes to the front of x's alternatives and every
        alternative naming the new digit leaves them."""
        new_digit, new_conf = self.alts[x][slot]
        f = Frame(list(self.digit), list(self.conf), list(self.alts))
        f.alts[x] = [(self.digit[x], self.conf[x])] + [a for a in self.alts[x] if a[0] != new_digit]
        f.digit[x], f.conf[x] = new_digit, new_conf
        return f


def validate(digit):
    """-> (number of conflicts, conflicts naming each cell [81], the conflicted cells in the order they are first named).
    A conflict is a (unit, digit > 0) with two or more cells; within a unit, digits in order of first appearance."""
    n, count, named = 0, [0] * 81, []
    for unit in UNITS:
        where = {}
        for x in unit:
            if digit[x] > 0:
                where.setdefault(digit[x], []).append(x)
        for cells in where.values():
            if len(cells) >= 2:
                n += 1
                for x in cells:
                    count[x] += 1
                    if x not in named:
                        named.append(x)
    return n, count, named


def score(frame, num_conflicts, mutant=None, scored=None):
    """Lower is better.  Every operation is one IEEE double operation; the sum is exact (see the module docstring) so its order is
    free.  scored: a list that receives the confidences summed, in order."""
    filled = [x for x in range(81) if frame.digit[x] > 0]
    if scored is not None:
        scored.append([frame.conf[x] for x in filled])
    total = np.float32(0.0) if mutant == "f32_sum" else 0.0
    for x in filled:
        total = total + (np.float32(frame.conf[x]) if mutant == "f32_sum" else frame.conf[x])
    total = float(total)
    if mutant == "f32_score":
        avg = np.float32(total) / np.float32(len(filled)) if filled else np.float32(0.0)
        return float(np.float32(num_conflicts * 100) + (np.float32(1.0) - avg) * np.float32(10.0))
    avg = total / len(filled) if filled else 0.0
    return float(num_conflicts * 100) + (1.0 - avg) * 10.0


def candidates(frame, min_alt, mutant=None):
    """-> ([(cell, slot)] of the first 10 corrections to try, how many there were before the cut)."""
    _, count, named = validate(frame.digit)
    keyed = []
    for order, x in enumerate(named):
        for slot, (d, p) in enumerate(frame.alts[x]):
            if d != frame.digit[x] and (np.float32(p) >= np.float32(min_alt) if mutant == "f32_threshold" else p >= min_alt):
                keyed.append(((-count[x], frame.conf[x], -p, order, slot), x, slot))
    keyed.sort(key=lambda t: t[0])
    return [(x, slot) for _, x, slot in keyed[:10]], len(keyed)


def smallest_by_score(scores, n):
    """Which of the paths with these scores (in evaluation order) form the next beam, in beam order: what CPython's
    heapq.nsmallest(n, paths) returns for objects that compare by score alone.  With n or fewer paths that is a stable sort.  With more
    it is NOT the first n of a stable sort: nsmallest keeps a max-heap of n (path, arrival number) pairs, the pairs compare by score
    only since no two paths are equal, and the result is the heap's array stably sorted by score -- equal scores come out in heap
    layout order, and which of several equal worst paths a better one evicts is the heap's choice too."""
    m = len(scores)
    if n >= m:
        return sorted(range(m), key=lambda i: scores[i])
    heap = list(range(n))

    def settle(pos):
        """heapq._siftup_max: the larger child (the right one when equal) moves up until a leaf, then the item climbs back while its
        parent is strictly smaller."""
        start, item = pos, heap[pos]
        child = 2 * pos + 1
        while child < n:
            if child + 1 < n and not scores[heap[child + 1]] < scores[heap[child]]:
                child += 1
            heap[pos] = heap[child]
            pos, child = child, 2 * child + 1
        while pos > start and scores[heap[(pos - 1) >> 1]] < scores[item]:
            heap[pos] = heap[(pos - 1) >> 1]
            pos = (pos - 1) >> 1
        heap[pos] = item

    for pos in reversed(range(n // 2)):
        settle(pos)
    for i in range(n, m):
        if scores[i] < scores[heap[0]]:
            heap[0] = i
            settle(0)
    return sorted(heap, key=lambda i: scores[i])


def resolve_frame(index, prob, beam_width=5, max_corrections=3, min_alt=0.1, mutant=None, scored=None):
    """One frame -> dict of its outputs (the fields of Context.resolve_conflicts) plus `stats` for the golden set's coverage checks:
    (depth that succeeded or 0, beam ran empty, most candidates of a path before the cut, most invalid paths of a depth)."""
    start = Frame.from_arrays(index, prob)
    before, _, _ = validate(start.digit)
    if scored is not None and before:
        score(start, before, scored=scored)             # the reference scores the input too (and never reads that score)
    explored, most_cand, most_invalid = 1, 0, 0
    if before == 0:
        return _result(start, [], True, before, explored, 0.0, index.shape[1], (0, 0, 0, 0))
    beam = [(start, [])]
    for depth in range(max_corrections):
        invalid, best = [], None
        for frame, made in beam:
            cands, total = candidates(frame, min_alt, mutant)
            most_cand = max(most_cand, total)
            for x, slot in cands:
                child = frame.corrected(x, slot)
                corr = made + [(x, frame.digit[x], child.digit[x], frame.conf[x], child.conf[x])]
                explored += 1
                nconf = validate(child.digit)[0]
                s = score(child, nconf, mutant, scored)
                if nconf == 0:
                    if best is None or s < best[0]:
                        best = (s, child, corr, explored)
                else:
                    invalid.append((s, None, child, corr))
        if best is not None:
            return _result(best[1], best[2], True, before, best[3], best[0], index.shape[1], (depth + 1, 0, most_cand, most_invalid))
        most_invalid = max(most_invalid, len(invalid))
        beam = [(invalid[i][2], invalid[i][3]) for i in smallest_by_score([t[0] for t in invalid], beam_width)]
        if not beam:
            return _result(start, [], False, before, explored, 0.0, index.shape[1], (0, 1, most_cand, most_invalid))
    frame, made = beam[0]
    return _result(frame, made, False, before, explored, 0.0, index.shape[1], (0, 0, most_cand, most_invalid))


def _result(frame, made, success, before, explored, s, k, stats):
    after, count, _ = validate(frame.digit)
    index = np.full((81, k), PAD_INDEX, np.uint8)
    prob = np.full((81, k), PAD_PROB, np.float32)
    index[:, 0], prob[:, 0] = frame.digit, frame.conf
    for x in range(81):
        for j, (d, p) in enumerate(frame.alts[x]):
            index[x, 1 + j], prob[x, 1 + j] = d, p
    cells = np.zeros((3, 3), np.uint8)
    cconf = np.zeros((3, 2), np.float32)
    for i, (x, old, new, old_conf, new_conf) in enumerate(made):
        cells[i], cconf[i] = (x, old, new), (old_conf, new_conf)
    return {"digits": index[:, 0].copy(), "conf": prob[:, 0].copy(), "index": index, "prob": prob, "success": np.uint8(success),
            "num_conflicts_before": np.int32(before), "num_conflicts_after": np.int32(after), "conflict_count": np.array(count, np.uint8),
            "n_corrections": np.uint8(len(made)), "corr_cells": cells, "corr_conf": cconf, "paths_explored": np.int32(explored),
            "score": np.float64(s), "stats": np.array(stats, np.int32)}


FIELDS = ("digits", "conf", "index", "prob", "success", "num_conflicts_before", "num_conflicts_after", "conflict_count", "n_corrections",
          "corr_cells", "corr_conf", "paths_explored", "score")


def resolve(index, prob, beam_width=5, max_corrections=3, min_alt=0.1, mutant=None, scored=None):
    """index u8 [n,81,k], prob f32 [n,81,k] -> dict of stacked arrays, FIELDS plus `stats` [n,4]."""
    index, prob = np.asarray(index, np.uint8), np.asarray(prob, np.float32)
    per = [resolve_frame(index[i], prob[i], beam_width, max_corrections, min_alt, mutant, scored) for i in range(index.shape[0])]
    return {key: np.stack([r[key] for r in per]) for key in FIELDS + ("stats",)}


# ---- the seeded frame generator ------------------------------------------------------------------------------------------------------
# confidences are integers / 4096: exact in f32, the same on every platform, and often equal (the tie rules).  410/4096 is the
# smallest such value >= 0.1 and 409/4096 the largest below it.
_TOP = (1229, 1638, 2048, 2458, 2867, 3277)
_ALT1 = (409, 410, 512, 614, 819, 1024)
_ALT2 = (205, 409, 410, 512)
GOLDEN_SEED, GOLDEN_N = 20, 512


def _solved(rs):
    g = np.array([[(3 * (r % 3) + r // 3 + c) % 9 + 1 for c in range(9)] for r in range(9)])
    g = (rs.permutation(9) + 1)[g - 1]
    rows = np.concatenate([3 * b + rs.permutation(3) for b in rs.permutation(3)])
    cols = np.concatenate([3 * b + rs.permutation(3) for b in rs.permutation(3)])
    return g[rows][:, cols].reshape(81)


def _peers(x):
    return sorted({y for u in UNITS if x in u for y in u} - {x})


def frames(seed, n, k=3):
    """n frames of a recogniser's top-k output: a solved grid under seeded permutations with about 50 cells blank, then 0-5 cells
    misread as a digit one of their peers shows; the true digit is the misread cell's alternative 1 or 2, or not among them.
    -> (index u8 [n,81,k], prob f32 [n,81,k])."""
    rs = np.random.RandomState(seed)
    index = np.zeros((n, 81, k), np.uint8)
    prob = np.zeros((n, 81, k), np.float32)
    for f in range(n):
        truth = _solved(rs)
        digit = truth.copy()
        digit[rs.permutation(81)[:50]] = 0
        weak = rs.randint(0, 12) == 0                         # a frame whose alternatives are all below 0.1: nothing to try
        wrong = {}
        for _ in range(rs.randint(0, 6)):
            filled = [x for x in range(81) if digit[x] > 0 and x not in wrong]
            x = filled[rs.randint(0, len(filled))]
            others = [y for y in _peers(x) if digit[y] > 0 and digit[y] != digit[x] and y not in wrong]
            if not others:
                continue
            wrong[x] = int(digit[x])
            digit[x] = digit[others[rs.randint(0, len(others))]]
        for x in range(81):
            d = int(digit[x])
            rest = [v for v in rs.permutation(10) if v != d]
            if x in wrong:
                where = rs.randint(0, 3)                      # slot 1, slot 2, absent
                rest = [v for v in rest if v != wrong[x]]
                if where < k - 1:
                    rest.insert(where, wrong[x])
            p = [_TOP[rs.randint(0, 3 if x in wrong else len(_TOP))], _ALT1[rs.randint(0, len(_ALT1))], _ALT2[rs.randint(0, len(_ALT2))]]
            if weak:
                p[1], p[2] = min(p[1], 409), min(p[2], 409)
            p[2] = min(p[2], p[1])
            p += [102] * max(0, k - 3)
            index[f, x] = [d] + rest[:k - 1]
            prob[f, x] = np.array(p[:k], np.float32) / np.float32(4096)
    return index, prob


# ---- real probabilities: the top-k of a float64 softmax over generated logits, rounded to f32 -----------------------------------------
REAL_SEED, REAL_N = 41, 256
REAL_VARIANTS = {"real_k2": (42, 32, 2), "real_k4": (43, 32, 4)}          # name -> (seed, n, k)
DOMAIN_FLOOR = 2.0 ** -18              # see the module docstring


def softmax_topk(logits, k):
    """Float64 softmax of f32 logits [..., 10] rounded to f32, then the k largest by a stable sort (equal probabilities: lowest class
    first) -> (index u8 [..., k], prob f32 [..., k]).  The denominator is math.fsum, which is correctly rounded whatever the order:
    cells that hold the same ten logits under different classes get bit-equal probabilities."""
    z = np.asarray(logits, np.float32).astype(np.float64)
    e = np.exp(z - z.max(-1, keepdims=True))
    den = np.array([math.fsum(row) for row in e.reshape(-1, 10)]).reshape(e.shape[:-1] + (1,))
    p = (e / den).astype(np.float32)
    order = np.argsort(-p, axis=-1, kind="stable")[..., :k]
    return order.astype(np.uint8), np.take_along_axis(p, order, -1)


def real_logits(seed, n):
    """Logits f32 [n,81,10] of n frames built as `frames` builds them (solved grid, about 50 blanks, 0-5 misread cells), ten normal
    draws (sigma 4) per cell, sorted, the largest given to the digit the cell shows and the true digit of a misread cell placed at
    rank 1, 2 or beyond 4.  Shapes: a misread cell is unsure (draws scaled by 0.08-0.3: alternatives around 0.1-0.3); other cells are
    confident (gap 20-30 to the runner-up: a tail that is tiny, not zero), near-uniform (scaled by 0.04: top-1 0.11-0.2) or as drawn;
    one frame in four is unsure everywhere (many eligible alternatives: long candidate lists, full beams), one in twelve confident
    everywhere (nothing to try).  In the last n // 8 frames every conflicted cell holds a copy of one cell's ten logits, each under
    its own classes: bit-equal full-mantissa confidences for the tie rules."""
    rs = np.random.RandomState(seed)
    out = np.zeros((n, 81, 10), np.float32)
    for f in range(n):
        truth = _solved(rs)
        digit = truth.copy()
        digit[rs.permutation(81)[:50]] = 0
        mood = rs.randint(0, 12)                              # 0: confident everywhere, 1-3: unsure everywhere
        wrong = {}
        for _ in range(rs.randint(0, 6)):
            filled = [x for x in range(81) if digit[x] > 0 and x not in wrong]
            x = filled[rs.randint(0, len(filled))]
            others = [y for y in _peers(x) if digit[y] > 0 and digit[y] != digit[x] and y not in wrong]
            if not others:
                continue
            wrong[x] = int(digit[x])
            digit[x] = digit[others[rs.randint(0, len(others))]]
        conflicted = validate([int(d) for d in digit])[2] if f >= n - n // 8 else []
        shared = None
        for x in range(81):
            d = int(digit[x])
            v = np.sort(rs.randn(10) * 4.0)[::-1].copy()
            shape = rs.rand()
            if mood == 0 or (x not in wrong and mood > 3 and shape < 0.5):
                v[0] = v[1] + 20.0 + 10.0 * rs.rand()
            elif x in wrong:
                v *= (0.08, 0.15, 0.3)[rs.randint(0, 3)]
            elif mood <= 3:
                v *= (0.03, 0.06, 0.12)[rs.randint(0, 3)]
            elif shape < 0.65:
                v *= 0.04
            v[0] += 0.05
            v = v.astype(np.float32)
            if x in conflicted:
                shared = v if shared is None else shared
                v = shared
            rest = [c for c in rs.permutation(10) if c != d]
            if x in wrong:
                rest.remove(wrong[x])
                rest.insert((0, 1, 3 + rs.randint(0, 5))[rs.randint(0, 3)], wrong[x])
            out[f, x, [d] + rest] = v
    return out


def real_frames(seed, n, k=3):
    """`frames` with real probabilities: softmax_topk of real_logits -> (index u8 [n,81,k], prob f32 [n,81,k])."""
    return softmax_topk(real_logits(seed, n), k)


# ---- the eligibility threshold where f32 rounds the wrong way -----------------------------------------------------------------------
# np.float32(0.1) lies above 0.1, so at the default an f32 comparison and a double one agree on every f32.  These thresholds round
# DOWN to f32: an alternative of exactly np.float32(m) is below m in doubles (not eligible) and passes an f32 comparison.
MINALT = tuple(m for m in (0.7, 0.3, 0.45, 0.35) if float(np.float32(m)) < m)
MINALT_SEED, MINALT_GENERATED, MINALT_CRAFTED = 44, 16, 6


def minalt_frames(m, k=3):
    """The frames run with min_alternative_confidence = m: MINALT_GENERATED real frames, then MINALT_CRAFTED frames whose deciding
    alternative is exactly np.float32(m), then the same frames with it one ulp above.  A crafted frame is a valid real frame in which
    a filled cell is given the digit of a confident peer and its true digit as alternative 1 with the deciding probability; every other
    confidence stays as the softmax made it (the peer's alternatives are far below m: the deciding one is the frame's only candidate).
    -> (index, prob, rows of the exact frames, rows of the frames one ulp above)"""
    gi, gp = real_frames(MINALT_SEED, MINALT_GENERATED, k)
    pool_i, pool_p = real_frames(MINALT_SEED + 1, 16 * MINALT_CRAFTED, k)
    at = np.float32(m)
    crafted = []
    for f in range(pool_i.shape[0]):
        digit = [int(v) for v in pool_i[f, :, 0]]
        if validate(digit)[0]:
            continue
        pairs = [(x, y) for x in range(81) for y in _peers(x) if digit[x] > 0 and digit[y] > 0 and pool_p[f, y, 1] < 0.01
                 and pool_p[f, x, 0] != at and all(digit[z] != digit[y] for z in _peers(x) if z != y)]
        if pairs and len(crafted) < MINALT_CRAFTED:
            x, y = pairs[len(crafted) % len(pairs)]
            ci, cp = pool_i[f].copy(), pool_p[f].copy()
            others = [c for c in range(10) if c not in (digit[x], digit[y])]
            ci[x, :] = ([digit[y], digit[x]] + others)[:k]
            cp[x, 1] = at
            cp[x, 2:] = np.minimum(cp[x, 2:], np.float32(0.01) * pool_p[f, x, 0])
            crafted.append((ci, cp))
    assert len(crafted) == MINALT_CRAFTED
    above = [(ci, cp.copy()) for ci, cp in crafted]
    for _, cp in above:
        cp[cp == at] = np.nextafter(at, np.float32(1))
    index = np.concatenate([gi] + [c[0][None] for c in crafted + above])
    prob = np.concatenate([gp] + [c[1][None] for c in crafted + above])
    exact = np.arange(MINALT_GENERATED, MINALT_GENERATED + MINALT_CRAFTED)
    return index, prob, exact, exact + MINALT_CRAFTED


def minalt_name(m):
    return "real_minalt." + repr(m).replace(".", "p")


# ---- crafted frames: the smallest inputs at which each rule can go wrong ---------------------------------------------------------------
def _frame(cells, k=3):
    """cells: {(row, col): (digit, conf, [(alt digit, alt prob), ...])}; an int probability is a count of 1/4096, a float is rounded
    to f32.  Every other cell is empty with alternatives far below 0.1."""
    def p32(v):
        return np.float32(v) / np.float32(4096) if isinstance(v, int) else np.float32(v)
    index = np.zeros((81, k), np.uint8)
    prob = np.zeros((81, k), np.float32)
    index[:, 1:] = np.arange(1, k)
    prob[:] = [p32(v) for v in (3686, 41, 20, 10)[:k]]
    for (r, c), (d, conf, alts) in cells.items():
        index[9 * r + c] = [d] + [a for a, _ in alts][:k - 1]
        prob[9 * r + c] = [p32(conf)] + [p32(p) for _, p in alts][:k - 1]
    return index[None], prob[None]


_W = [(1, 205), (2, 102)]          # alternatives below 0.1


def crafted_cases():
    """name -> (index [1,81,3], prob [1,81,3]); all run with beam 5, 3 corrections."""
    cases = {}
    cases["valid"] = _frame({(0, 0): (5, 3277, _W), (0, 1): (3, 2048, _W), (4, 4): (5, 2458, _W)})
    # the reference's own self-test (conflict_resolver.py:293-322): one correction, (0,3) 5 -> 8
    cases["selftest"] = _frame({(0, 0): (5, 0.95, [(3, 0.03), (6, 0.02)]), (0, 1): (3, 0.88, [(8, 0.05), (2, 0.04)]),
                                (0, 3): (5, 0.6, [(8, 0.25), (9, 0.10)])})
    cases["all_weak"] = _frame({(0, 0): (5, 2048, [(1, 409), (2, 409)]), (0, 3): (5, 2458, [(3, 409), (4, 205)])})
    cases["count3"] = _frame({(0, 0): (5, 2048, _W), (0, 5): (5, 2048, _W), (5, 0): (5, 2048, _W), (1, 1): (5, 2048, _W)})
    cases["three_in_row_weak"] = _frame({(0, 0): (7, 2048, _W), (0, 3): (7, 2458, _W), (0, 6): (7, 2867, _W)})
    cases["three_in_row"] = _frame({(0, 0): (7, 2048, [(1, 819), (2, 410)]), (0, 3): (7, 2458, [(3, 819), (4, 409)]),
                                    (0, 6): (7, 2867, [(6, 819), (8, 410)])})
    # bit-equal confidences and alternative confidences: two valid paths of equal score, the first-named cell's wins with paths_explored 2
    cases["tie_first_named"] = _frame({(0, 0): (5, 2048, [(1, 819), (2, 205)]), (0, 3): (5, 2048, [(2, 819), (1, 205)])})
    # named order is not cell order: the row conflict of (5,0) is reported before the column conflict of (1,3).  Needs exactly 2 corrections,
    # reachable in either order: the depth-1 paths tie, and so do the two valid depth-2 paths
    cases["named_order_two"] = _frame({(5, 0): (5, 2048, [(1, 819), (2, 205)]), (5, 4): (5, 2048, [(2, 819), (1, 205)]),
                                       (1, 3): (6, 2048, [(3, 819), (4, 205)]), (7, 3): (6, 2048, [(4, 819), (3, 205)])})
    cases["exact_two"] = _frame({(0, 0): (5, 1229, [(1, 1024), (2, 205)]), (0, 3): (5, 3277, _W),
                                 (4, 1): (6, 1638, [(3, 614), (4, 512)]), (4, 7): (6, 3277, _W)})
    cases["exact_three"] = _frame({(0, 0): (5, 1229, [(1, 1024), (2, 205)]), (0, 3): (5, 3277, _W),
                                   (3, 1): (6, 1638, [(3, 614), (4, 512)]), (3, 7): (6, 3277, _W),
                                   (6, 2): (8, 2048, [(9, 819), (7, 410)]), (6, 5): (8, 2867, [(7, 410), (9, 409)])})
    # four independent conflicts, everything equal: 16 candidates cut to 10, 10 invalid paths cut to 5 among ties, success False after depth 3
    cases["need_four"] = _frame({(r, c): (d, 2048, [(a, 819), (b, 512)]) for r, c, d, a, b in
                                 ((0, 0, 5, 1, 2), (0, 3, 5, 2, 1), (2, 1, 6, 3, 4), (2, 7, 6, 4, 3),
                                  (4, 2, 7, 1, 3), (4, 5, 7, 3, 1), (6, 4, 8, 2, 4), (6, 8, 8, 4, 2))})
    # (0,0) 5 -> 7 collides with (0,6); at the next depth the best candidate of that path puts the 5 back
    cases["restore"] = _frame({(0, 0): (5, 3277, [(7, 614), (9, 205)]), (0, 3): (5, 3686, _W), (0, 6): (7, 3686, _W)})
    cases["zero_alternative"] = _frame({(0, 0): (5, 2048, [(0, 819), (3, 205)]), (0, 3): (5, 3277, _W)})
    # nine conflicted cells with two eligible alternatives each: 18 candidates, 10 kept
    cases["cut_at_ten"] = _frame({(0, c): (4, 1229 + 409 * (c % 3), [(1 + (c + 1) % 9, 819 - 10 * c), (1 + (c + 5) % 9, 410)]) for c in range(9)})
    return cases


# generated frames under other arguments: name -> (seed, n, k, beam_width, max_corrections)
VARIANTS = {"k1": (31, 32, 1, 5, 3), "k2": (32, 32, 2, 5, 3), "k4": (33, 32, 4, 5, 3),
            "beam1": (34, 48, 3, 1, 3), "beam6": (34, 48, 3, 6, 3), "max0": (34, 48, 3, 5, 0), "max1": (34, 48, 3, 5, 1)}
