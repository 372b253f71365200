"""CPU: the plain-Python restatement of run_v2's constraint propagation (tests/constraint_ref.py) == the reference's own results
(tests/golden/constraint_goldens.npz), every field; and the restatement's integer replay of list(set(...)) == the running
interpreter's set.  The second is the test that notices a Python whose set or tuple hash behaves differently from what
csrc/k10_propagate.hip replays."""
import os

import numpy as np
import pytest

import constraint_ref as cr


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "constraint_goldens.npz"))


@pytest.fixture(scope="module")
def generated():
    digits, conf = cr.frames()
    trace = []
    return digits, conf, cr.propagate(digits, conf, trace=trace), trace


def same(got, golden, prefix, what):
    for key in cr.FIELDS:
        a, b = got[key], golden[f"{prefix}.{key}"]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = sorted({int(i[0]) for i in np.argwhere(a != b)})
            raise AssertionError(f"{what}: {key} differs in {len(bad)} frames, first {bad[:8]}: got {a[bad[0]].tolist()} want {b[bad[0]].tolist()}")


def test_generator_is_what_the_goldens_were_made_from(golden):
    assert (int(golden["seed"]), int(golden["per_kind"])) == (cr.GOLDEN_SEED, cr.PER_KIND)
    assert golden["gen.grid"].shape == (4 * cr.PER_KIND, 81)


def test_restatement_equals_the_reference_on_generated_frames(generated, golden):
    same(generated[2], golden, "gen", "generated frames")


@pytest.mark.parametrize("name", sorted(cr.crafted_cases()))
def test_restatement_equals_the_reference_on_crafted_cases(golden, name):
    digits, conf, it = cr.crafted_cases()[name]
    same(cr.propagate(digits, conf, it), golden, f"case.{name}", name)


def test_goldens_cover_the_order_rule(golden):
    """Recorded from the reference alone: enough frames on which a sorted-order implementation gives another result, some of them
    another is_valid, none among the consistent frames; and tables that grew to 32 and to 128 slots."""
    n = cr.PER_KIND
    assert golden["gen.order_differs"].sum() >= 25 and golden["gen.valid_differs"].sum() >= 3 and golden["gen.order_differs"][:n].sum() == 0
    assert golden["gen.is_valid"][:n].all() and (golden["gen.is_valid"][n:] == 0).sum() >= 25
    assert (golden["gen.distinct"] >= 5).any() and (golden["gen.distinct"] >= 19).any()


def test_a_sorted_order_restatement_fails_where_the_goldens_say_so(generated, golden):
    digits, conf, want, _ = generated
    rows = np.nonzero(golden["gen.order_differs"])[0][:32]
    got = cr.propagate(digits[rows], conf[rows], order=sorted)
    differs = [any(got[key][i].tobytes() != want[key][f].tobytes() for key in cr.FIELDS) for i, f in enumerate(rows)]
    assert all(differs)


def test_crafted_cases_show_what_they_are_for():
    got = {name: cr.propagate(*case) for name, case in cr.crafted_cases().items()}

    def one(name, key):
        return got[name][key][0].tolist()
    assert (one("empty", "is_valid"), one("empty", "iterations"), one("empty", "n_resolved")) == (1, 1, 0) and set(one("empty", "candidates")) == {cr.ALL}
    assert (one("full", "is_valid"), one("full", "iterations"), one("full", "n_resolved")) == (1, 1, 0)
    assert one("selftest", "is_valid") == 1 and 0 not in one("selftest", "grid") and one("selftest", "n_resolved") == 51
    assert one("selftest_conf", "is_fixed")[:6] == [0, 0, 0, 0, 1, 0] and one("selftest", "is_fixed")[:3] == [1, 1, 0]
    assert (one("naked_peers_same_digit", "is_valid"), one("naked_peers_same_digit", "contradiction_cell"), one("naked_peers_same_digit", "iterations")) == (0, 1, 1)
    assert one("naked_peers_same_digit", "resolved")[:2] == [[0, 1], [255, 255]] and one("naked_peers_same_digit", "grid")[:2] == [1, 0]
    trace = []
    cr.propagate(*cr.crafted_cases()["two_hidden_one_cell"], trace=trace)
    assert {(0, 0, 1), (0, 0, 2)} <= set(trace[0]) and trace[0].count((0, 0, 1)) == 2
    first = [e for e in cr.set_order(trace[0])[0] if e[:2] == (0, 0)][0][2]
    assert one("two_hidden_one_cell", "grid")[0] == first and one("two_hidden_one_cell", "is_valid") == 1
    trace = []
    cr.propagate(*cr.crafted_cases()["hidden_undone"], trace=trace)
    order = [e for e in cr.set_order(trace[0])[0] if e in ((0, 0, 1), (1, 1, 1))]
    assert len(order) == 2 and one("hidden_undone", "is_valid") == 0 and one("hidden_undone", "iterations") == 1
    assert one("hidden_undone", "contradiction_cell") == 9 * order[1][0] + order[1][1] and one("hidden_undone", "grid")[9 * order[0][0] + order[0][1]] == 1
    assert one("filled_emptied", "candidates")[0] == one("filled_emptied", "candidates")[5] == 0 and one("filled_emptied", "is_valid") == 1
    assert one("filled_emptied", "candidates")[40] == 1 << 3
    assert (one("no_candidates_on_entry", "is_valid"), one("no_candidates_on_entry", "contradiction_cell"), one("no_candidates_on_entry", "iterations")) == (0, 0, 1)
    assert one("no_candidates_on_entry", "candidates")[0] == 0
    assert one("selftest", "iterations") > 3
    for it in (1, 2):
        assert (one(f"selftest_max{it}", "iterations"), one(f"selftest_max{it}", "is_valid")) == (it, 1) and 0 in one(f"selftest_max{it}", "grid")
    assert one("selftest_max1", "n_resolved") < one("selftest_max2", "n_resolved") < 51


def test_tuple_hash_is_the_interpreters():
    rs = np.random.RandomState(5)
    for _ in range(2000):
        t = tuple(int(v) for v in rs.randint(0, 10, size=3))
        assert cr.tuple_hash(t) == hash(t) % (1 << 64)


def test_set_order_is_the_interpreters_on_the_generated_frames(generated):
    trace = generated[3]
    assert len(trace) > 1000 and max(len(set(e)) for e in trace) >= 19
    sizes = set()
    for entries in trace:
        got, size = cr.set_order(entries)
        assert got == list(set(entries))
        sizes.add(size)
    assert {8, 32, 128} <= sizes


def test_set_order_is_the_interpreters_on_random_lists():
    """1000 lists of 1..243 (r, c, v) tuples with repeats, as many as a pass can produce: every table size up to 512 slots."""
    rs = np.random.RandomState(7)
    sizes = set()
    for i in range(1000):
        n = 1 + i % 243
        pool = [(int(r), int(c), int(v)) for r, c, v in zip(rs.randint(0, 9, n), rs.randint(0, 9, n), rs.randint(1, 10, n))]
        entries = [pool[j] for j in rs.randint(0, n, n)] if i % 3 == 0 else pool
        got, size = cr.set_order(entries)
        assert got == list(set(entries)), (i, n)
        sizes.add(size)
    assert sizes == {8, 32, 128, 512}
