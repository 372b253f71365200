"""Plain-Python restatement of run_v2's constraint propagation (pipeline/constraint_resolver.py:48-267 as pipeline/run_v2.py:373-391
calls it), arrays in, arrays out, and the seeded frame generator the propagation tests share.  Written from the rules in DESIGN.md
("K10"), not from csrc/k10_propagate.hip: one cell at a time, candidates as integers, and no `set` anywhere: the order in which the
reference's list(set(hidden singles)) hands the entries back is computed here with integers (tuple_hash, set_order), so that a test
can hold it against the running interpreter's own set.

A frame is digits u8 [81] (0 = empty) and, optionally, conf f32 [81].  A cell's candidates are a bit mask: bit d set = d possible.
"""
import numpy as np

ROWS = [[9 * r + c for c in range(9)] for r in range(9)]
COLS = [[9 * r + c for r in range(9)] for c in range(9)]
BOXES = [[9 * (3 * (b // 3) + i) + 3 * (b % 3) + j for i in range(3) for j in range(3)] for b in range(9)]
UNITS = ROWS + COLS + BOXES            # the order find_hidden_singles walks them in
PEERS = [sorted({y for u in UNITS if x in u for y in u} - {x}) for x in range(81)]
ALL = 0x3FE                            # candidates 1..9
NONE = 255                             # no contradiction cell; an unused entry of `resolved`

FIELDS = ("grid", "candidates", "is_valid", "iterations", "contradiction_cell", "n_resolved", "resolved", "is_fixed")

# ---- the order of list(set(entries)) in CPython 3.8+ ----------------------------------------------------------------------------------
_M64 = (1 << 64) - 1
_P1, _P2, _P5 = 11400714785074694791, 14029467366897019727, 2870177450012600261


def tuple_hash(items):
    """hash(tuple(items)) for small non-negative ints (Objects/tupleobject.c, the xxHash-style mix), as the unsigned 64-bit value
    the set probes with."""
    acc = _P5
    for v in items:
        acc = (acc + v * _P2) & _M64                  # hash(v) == v for 0 <= v < 2**61 - 1
        acc = ((acc << 31) | (acc >> 33)) & _M64
        acc = (acc * _P1) & _M64
    acc = (acc + (len(items) ^ (_P5 ^ 3527539))) & _M64
    return 1546275796 if acc == _M64 else acc


def _slots(mask, h):
    """The slots set_add_entry / set_insert_clean (Objects/setobject.c) look at for hash h, in order: slot i and, where all of them
    lie inside the table, the 9 after it; then i = 5 i + 1 + (perturb >>= 5)."""
    i, perturb = h & mask, h
    while True:
        for j in range(10 if i + 9 <= mask else 1):
            yield i + j
        perturb >>= 5
        i = (i * 5 + 1 + perturb) & mask


def set_order(entries):
    """list(set(entries)) for a list of tuples of small ints, without a set: entries go in one by one (a duplicate is dropped); an
    entry that brings the table to fill * 5 >= mask * 3 makes it grow to the smallest power of two above 4 * used, the old entries
    re-inserted in slot order; the result is the table read from slot 0 up.  -> (the list, the table size at the end)."""
    mask, table, used = 7, [None] * 8, 0
    for e in entries:
        h = tuple_hash(e)
        for i in _slots(mask, h):
            if table[i] is None or table[i] == (h, e):
                break
        if table[i] is not None:
            continue
        table[i] = (h, e)
        used += 1
        if used * 5 >= mask * 3:
            size = 8
            while size <= used * 4:
                size <<= 1
            old, mask, table = table, size - 1, [None] * size
            for slot in old:
                if slot is not None:
                    for i in _slots(mask, slot[0]):
                        if table[i] is None:
                            break
                    table[i] = slot
    return [slot[1] for slot in table if slot is not None], mask + 1


# ---- propagation ----------------------------------------------------------------------------------------------------------------------
class _State:
    def __init__(self, digits):
        self.value = [int(v) for v in digits]
        self.cand = [(1 << v) if v else ALL for v in self.value]
        for x in range(81):                            # every filled cell takes its value from its peers, filled ones included
            if self.value[x]:
                self.eliminate(x, self.value[x])

    def eliminate(self, x, v):
        for y in PEERS[x]:
            self.cand[y] &= ~(1 << v)

    def place(self, x, v):
        """_set_cell on an empty cell -> False when v is not a candidate any more."""
        if not self.cand[x] >> v & 1:
            return False
        self.value[x], self.cand[x] = v, 1 << v
        self.eliminate(x, v)
        return True

    def naked(self):
        return [(x // 9, x % 9, self.cand[x].bit_length() - 1) for x in range(81) if not self.value[x] and bin(self.cand[x]).count("1") == 1]

    def hidden_list(self):
        """find_hidden_singles before its list(set(...)): rows, columns, boxes; digits ascending; a unit showing the digit is skipped."""
        out = []
        for unit in UNITS:
            for d in range(1, 10):
                if any(self.value[x] == d for x in unit):
                    continue
                where = [x for x in unit if not self.value[x] and self.cand[x] >> d & 1]
                if len(where) == 1:
                    out.append((where[0] // 9, where[0] % 9, d))
        return out


def propagate_one(digits, conf=None, max_iterations=100, order=None, trace=None):
    """One frame -> dict of FIELDS (scalars and arrays).  order: what turns the hidden-single list into the order it is applied in
    (default: set_order, the reference's); trace: a list that receives every pass's hidden-single list, before deduplication."""
    digits = np.asarray(digits, np.uint8).reshape(81)
    c = np.ones(81, np.float32) if conf is None else np.asarray(conf, np.float32).reshape(81)
    out = {"grid": digits.copy(), "candidates": np.zeros(81, np.uint16), "is_valid": np.uint8(0), "iterations": np.int32(0),
           "contradiction_cell": np.uint8(NONE), "n_resolved": np.uint8(0), "resolved": np.full((81, 2), NONE, np.uint8),
           "is_fixed": np.array([digits[x] > 0 and float(c[x]) > 0.9 for x in range(81)], np.uint8)}
    if (digits > 9).any():                             # not a grid: reported invalid, nothing else computed
        return out
    s = _State(digits)
    done, iterations, bad = [], 0, None
    while iterations < max_iterations and bad is None:
        iterations += 1
        progress = False
        for r, col, v in s.naked():                    # found first, all of them; then applied in that order
            if not s.place(9 * r + col, v):
                bad = 9 * r + col
                break
            done.append((9 * r + col, v))
            progress = True
        if bad is not None:
            break
        entries = s.hidden_list()
        if trace is not None:
            trace.append(entries)
        for r, col, v in (order(entries) if order else set_order(entries)[0]):
            x = 9 * r + col
            if s.value[x]:
                continue                               # filled earlier in this pass
            if not s.place(x, v):
                bad = x
                break
            done.append((x, v))
            progress = True
        if bad is not None:
            break
        bad = next((x for x in range(81) if not s.value[x] and not s.cand[x]), None)
        if not progress:
            break
    out["grid"] = np.array(s.value, np.uint8)
    out["candidates"] = np.array(s.cand, np.uint16)
    out["is_valid"], out["iterations"] = np.uint8(bad is None), np.int32(iterations)
    out["contradiction_cell"] = np.uint8(NONE if bad is None else bad)
    out["n_resolved"] = np.uint8(len(done))
    for i, (x, v) in enumerate(done):
        out["resolved"][i] = (x, v)
    return out


def propagate(digits, conf=None, max_iterations=100, **kw):
    """digits u8 [n,81], conf f32 [n,81] or None -> dict of FIELDS, stacked over the frames."""
    digits = np.asarray(digits, np.uint8).reshape(-1, 81)
    rows = [propagate_one(digits[f], None if conf is None else conf[f], max_iterations, **kw) for f in range(digits.shape[0])]
    proto = propagate_one(np.zeros(81, np.uint8))
    return {key: np.stack([r[key] for r in rows]) if rows else np.zeros((0,) + np.shape(proto[key]), np.asarray(proto[key]).dtype) for key in FIELDS}


# ---- generated frames -----------------------------------------------------------------------------------------------------------------
GOLDEN_SEED, PER_KIND = 20260, 128
KINDS = ("consistent", "one_misread", "three_misread", "two_conflicting")
# confidences on both sides of is_fixed's `> 0.9`, which the reference evaluates on the double: float32(0.9) lies below 0.9
_CONF = np.array([0.5, 0.8999999, 0.9, 0.90000004, 0.99, 1.0], np.float32)


def _solved(rs):
    g = np.array([[(3 * (r % 3) + r // 3 + c) % 9 + 1 for c in range(9)] for r in range(9)])
    g = (rs.permutation(9) + 1)[g - 1]
    rows = np.concatenate([3 * b + rs.permutation(3) for b in rs.permutation(3)])
    cols = np.concatenate([3 * b + rs.permutation(3) for b in rs.permutation(3)])
    return g[rows][:, cols].reshape(81)


def frames(seed=GOLDEN_SEED, per_kind=PER_KIND):
    """per_kind frames of each of KINDS, kind after kind: a solved grid under seeded permutations with 30-57 cells blanked; then
    1 or 3 shown cells changed to another digit (a misreading, which may or may not show as a conflict), or 2 shown cells changed to
    a digit one of their shown peers has.  -> (digits u8 [4 * per_kind, 81], conf f32 [4 * per_kind, 81])."""
    rs = np.random.RandomState(seed)
    digits = np.zeros((4 * per_kind, 81), np.uint8)
    for f in range(4 * per_kind):
        kind = f // per_kind
        g = _solved(rs)
        g[rs.permutation(81)[:rs.randint(30, 58)]] = 0
        changed = []
        for _ in range((0, 1, 3, 2)[kind]):
            shown = [x for x in range(81) if g[x] and x not in changed]
            for x in (shown[i] for i in rs.permutation(len(shown))):
                seen = {int(g[y]) for y in PEERS[x] if g[y]}
                pick = sorted(seen - {int(g[x])}) if kind == 3 else sorted(set(range(1, 10)) - {int(g[x])})
                if pick:
                    g[x] = pick[rs.randint(0, len(pick))]
                    changed.append(x)
                    break
        digits[f] = g
    conf = _CONF[rs.randint(0, len(_CONF), size=digits.shape)]
    return digits, conf


# ---- crafted frames: the smallest inputs at which each rule can go wrong ---------------------------------------------------------------
SELFTEST = [[5, 3, 0, 0, 7, 0, 0, 0, 0], [6, 0, 0, 1, 9, 5, 0, 0, 0], [0, 9, 8, 0, 0, 0, 0, 6, 0],
            [8, 0, 0, 0, 6, 0, 0, 0, 3], [4, 0, 0, 8, 0, 3, 0, 0, 1], [7, 0, 0, 0, 2, 0, 0, 0, 6],
            [0, 6, 0, 0, 0, 0, 2, 8, 0], [0, 0, 0, 4, 1, 9, 0, 0, 5], [0, 0, 0, 0, 8, 0, 0, 7, 9]]   # constraint_resolver.py:328-338


def _grid(cells):
    g = np.zeros((1, 81), np.uint8)
    for (r, c), v in cells.items():
        g[0, 9 * r + c] = v
    return g


def crafted_cases():
    """name -> (digits u8 [1,81], conf f32 [1,81] or None, max_iterations)"""
    cases = {}
    cases["empty"] = (_grid({}), None, 100)
    cases["full"] = (_solved(np.random.RandomState(3)).astype(np.uint8)[None], None, 100)
    cases["selftest"] = (np.array(SELFTEST, np.uint8).reshape(1, 81), None, 100)
    cases["selftest_conf"] = (cases["selftest"][0], _CONF[np.arange(81) % len(_CONF)][None], 100)
    # (0,0) and (0,1) are both left with {1}: the first is placed, the second then finds its 1 gone
    row = {(0, c): c + 1 for c in range(2, 9)}
    cases["naked_peers_same_digit"] = (_grid({**row, (3, 0): 2, (6, 1): 2}), None, 100)
    # (0,0) is the only place for 1 in row 0 (and in box 0) and the only place for 2 in column 0: two entries, one cell
    cases["two_hidden_one_cell"] = (_grid({(0, 1): 8, (0, 2): 9, (1, 3): 1, (2, 6): 1, (1, 0): 6, (2, 0): 7, (3, 1): 2, (6, 2): 2}), None, 100)
    # 1 is a hidden single of row 0 at (0,0) and of column 1 at (1,1), which are peers: whichever the set hands back first is placed
    # and the other one fails
    cases["hidden_undone"] = (_grid({(0, 1): 8, (0, 2): 9, (0, 8): 7, (2, 4): 1, (3, 6): 1, (6, 7): 1, (5, 2): 1, (7, 1): 2, (8, 1): 3}), None, 100)
    # two 5s in a row empty each other's candidates; a filled cell without candidates is never looked at
    cases["filled_emptied"] = (_grid({(0, 0): 5, (0, 5): 5, (4, 4): 3}), None, 100)
    # (0,0) has no candidate before anything is placed
    cases["no_candidates_on_entry"] = (_grid({**{(0, c): c for c in range(1, 9)}, (1, 0): 9}), None, 100)
    cases["selftest_max1"] = (cases["selftest"][0], None, 1)
    cases["selftest_max2"] = (cases["selftest"][0], None, 2)
    return cases
