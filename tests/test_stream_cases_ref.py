"""CPU: the case table of tests/test_gpu_stream_order.py (tests/stream_cases.py) is fit for its purpose without a GPU: every case's inputs A and B
pass what the wrappers check of them, and the restatement tells them apart, so that a stale read of A where B was due cannot go unseen."""
import numpy as np
import pytest

import stream_cases as sc


def _differ(a, b):
    if isinstance(a, bytes) or isinstance(b, bytes):
        return a != b
    a, b = np.asarray(a), np.asarray(b)
    return a.shape != b.shape or a.tobytes() != b.tobytes()


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_inputs_are_valid_and_give_different_results(name):
    case = sc.by_name(name)
    A, B = case.inputs()
    sc.check_input(A)
    sc.check_input(B)
    if case.want is None:                                      # compared with an eager call on the GPU: the inputs at least differ
        assert all(_differ(A[k], B[k]) for k in A if not k.startswith("_")), "A and B share a buffer's contents"
        return
    wa, wb = case.want(A), case.want(B)
    assert len(wa) == len(wb) and any(_differ(x, y) for x, y in zip(wa, wb)), "want(A) == want(B)"
    if case.name in sc.CONTROLS:
        assert _differ(wa[0], wb[0])


def test_every_entry_is_in_exactly_one_list():
    assert len(set(sc.PURE) | set(sc.HOST)) == len(sc.CASES) == len(sc.PURE) + len(sc.HOST)
    assert set(sc.CONTROLS) <= {c.name for c in sc.CASES}
    assert sc.by_name("harris_corners").kind == "host" and sc.by_name("imencode").kind == "host"
    assert all(sc.by_name(n).kind == "decode" for n in sc.HOST if n.startswith("imdecode"))
