"""GPU (-m gpu): the context's grow-only device buffers (sv_scratch, csrc/sv_internal.h) over regrowth, reuse after the demand has shrunk,
and teardown.

Every user of a scratch buffer runs on one context at a small shape, then at a larger one (the buffer is freed and allocated anew), then
at the small one again (the larger buffer is reused, its old contents still in it).  Each result must be bit-equal to the same call on a
context that has done nothing else.  The memory tests read the device's free memory (torch.cuda.mem_get_info), after one pass over every
user on a throwaway context: the first launch of a kernel loads its code object, and torch's caching allocator takes its segments, both
out of the same free memory."""
import gc

import numpy as np
import pytest
import torch

import cnn_oracle
import jpeg_craft
import model_v3_ref

pytestmark = pytest.mark.gpu

SHAPES = ((1, 48, 64), (2, 96, 160))            # small, large: the frames of the K7, K11 and K13 cases
ORDER = (0, 1, 0)                               # small, large, small again
_RS = np.random.RandomState(20261)
GRAY = [_RS.randint(0, 256, s).astype(np.uint8) for s in SHAPES]
NOISE = [((_RS.rand(*s) < 0.45) * 255).astype(np.uint8) for s in SHAPES]
CELLS_F32 = _RS.rand(162, 1, 28, 28).astype(np.float32)
CELLS_V3 = model_v3_ref.inputs(5, 9)
_SD = {}


def _jpeg(width, height, seed):
    """A 4:2:0 file of random low-frequency coefficients: (height, width) is no multiple of the 16x16 MCU"""
    rs = np.random.RandomState(seed)
    mcus = -(-width // 16) * -(-height // 16)
    coef = np.zeros((6 * mcus, 64), np.int16)
    coef[:, 0] = rs.randint(-60, 61, len(coef))
    coef[:, 1:10] = rs.randint(-6, 7, (len(coef), 9))
    return jpeg_craft.write_jpeg(coef, np.full((3, 64), 8), width, height, "4:2:0")


JPEGS = [_jpeg(40, 24, 1), _jpeg(200, 120, 2)]


def _dev(a):
    return torch.from_numpy(a).cuda()


def _load_v1(c):
    if "v1" not in _SD:
        _SD["v1"] = cnn_oracle.random_state_dict(1234)
    c.load_state_dict(_SD["v1"])


def _load_v3(c):
    if "v3" not in _SD:
        _SD["v3"] = model_v3_ref.random_state_dict_v3(2024, True)       # the weights of tests/golden/model_v3_se.npz
    c.load_state_dict_v3(_SD["v3"])


def _harris(c, i):
    corners, counts = c.harris_corners(_dev(GRAY[i]), max_corners=50, min_distance=3)
    counts = counts.cpu().numpy()
    assert counts.min() > 0
    return (counts,) + tuple(corners[f, :n] for f, n in enumerate(counts))          # rows past a frame's count are not written


# name -> (what to load first, the call at shape index i); the results are tensors or tuples of them
USERS = {
    "k7_close_ellipse5": (None, lambda c, i: c.morphology(_dev(GRAY[i]), c.MORPH_CLOSE, c.SHAPE_ELLIPSE, 5)),
    "k7_clahe": (None, lambda c, i: c.clahe(_dev(GRAY[i]))),
    "k11_component_filter": (None, lambda c, i: c.component_filter(_dev(NOISE[i]), min_area_ratio=0.01)),
    "k13_harris": (None, _harris),
    "jpeg_imdecode": (None, lambda c, i: c.imdecode(JPEGS[i])),
    "cnn_forward": (_load_v1, lambda c, i: c.cnn_forward(_dev(CELLS_F32[:81 * (i + 1)]), want_digits=True)),
    "cnn3_forward": (_load_v3, lambda c, i: c.cnn3_forward(_dev(CELLS_V3[:(3, 9)[i]]), want_digits=True, want_features=True)),
}


def _host(out):
    torch.cuda.synchronize()
    return [np.asarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t) for t in (out if isinstance(out, tuple) else (out,))]


def _fresh(name, i):
    """What user `name` gives at shape i on a context of its own."""
    import sudoku_vision_amd as sva
    load, call = USERS[name]
    c = sva.Context()
    try:
        if load:
            load(c)
        return _host(call(c, i))
    finally:
        c.close()


def _exercise(c):
    """Every user on context c: small, large, small."""
    for load, call in USERS.values():
        if load:
            load(c)
        for i in ORDER:
            _host(call(c, i))


@pytest.mark.parametrize("name", list(USERS))
def test_grow_then_reuse_equals_fresh_context(name):
    import sudoku_vision_amd as sva
    load, call = USERS[name]
    want = [_fresh(name, i) for i in (0, 1)]
    assert any(w.size and w.any() for w in want[0]) and any(w.size and w.any() for w in want[1]), "the case computes nothing"
    c = sva.Context()
    try:
        if load:
            load(c)
        for step, i in enumerate(ORDER):
            got = _host(call(c, i))
            assert len(got) == len(want[i])
            for k, (g, w) in enumerate(zip(got, want[i])):
                assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, "step", step, "output", k)
    finally:
        c.close()


def _free_bytes():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


@pytest.fixture(scope="module")
def warmed():
    """Every kernel of the users has been launched once and every weight set packed once, on a context that is gone again."""
    import sudoku_vision_amd as sva
    c = sva.Context()
    _exercise(c)
    c.close()


def test_forward_after_reserve_allocates_nothing(warmed):
    """sv_ctx_reserve(162) sizes features / cells / cells2 and allocates the f32 input's range flag; the forward of 162 f32 cells (which
    uses that flag: CNN_AUTO) then takes no device memory.  Its outputs come out of blocks that torch already holds."""
    import sudoku_vision_amd as sva
    c = sva.Context()
    try:
        _load_v1(c)
        x = _dev(CELLS_F32)
        c.cnn_forward(x[:1], want_digits=True)             # one cell: scratch for one cell, and torch has a segment for the outputs
        torch.cuda.synchronize()
        c.reserve(162)
        before = torch.cuda.mem_get_info()[0]
        logits, digits, _ = c.cnn_forward(x, want_digits=True)
        torch.cuda.synchronize()
        after = torch.cuda.mem_get_info()[0]
        print(f"SCRATCH reserve(162) then forward(162): free {before} -> {after}")
        assert after == before
        want = _fresh("cnn_forward", 1)
        assert logits.cpu().numpy().tobytes() == want[0].tobytes() and digits.cpu().numpy().tobytes() == want[1].tobytes()
    finally:
        c.close()


def test_close_gives_all_device_memory_back(warmed):
    """A context that has grown every buffer it has (each user, small, large, small) and is then closed leaves the device's free memory
    where it was before the context was created: sv_ctx_destroy frees every sv_scratch and every weight image.  Equality is what the
    code before sv_scratch satisfied on an MI355X (its sv_ctx_destroy named ten pointers one by one), with torch's cache emptied on
    both sides of the comparison."""
    import sudoku_vision_amd as sva
    before = _free_bytes()
    c = sva.Context()
    _exercise(c)
    held = _free_bytes()
    assert held < before, "the context holds no device memory: the test measures nothing"
    c.close()
    del c
    after = _free_bytes()
    print(f"SCRATCH free before the context {before}, with it {held}, after close {after}")
    assert after == before
