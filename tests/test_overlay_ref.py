"""CPU: the overlay's restatement (tests/overlay_ref.py) notices every mistake it names; the host side of the overlay -- the forward
homography, the default font, overlay_cells -- is right; and the definition draws digits that can be told apart."""
import os
import sys

import numpy as np
import pytest

import overlay_ref as ov
import warp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sva():
    import __graft_entry__ as g
    import sudoku_vision_amd as sva
    if not os.path.exists(sva._native.LIB_PATH):
        g.build()
    sva._native.lib()
    return sva


@pytest.fixture(scope="module")
def references():
    return {g.name: ov.reference(g) for g in ov.GEOMETRIES}


@pytest.mark.parametrize("mutation", sorted(ov.MUTATIONS))
def test_every_mutation_changes_some_geometry(references, mutation):
    hit = [g.name for g in ov.GEOMETRIES if (ov.reference(g, mutation) != references[g.name]).any()]
    assert hit, f"{mutation}: {ov.MUTATIONS[mutation]} -- no geometry notices it"


def test_margin_shortcuts_are_invisible_with_a_margin(references):
    """The two shortcuts the kernel takes are exact on every atlas the library accepts: only `no_margin` tells them apart."""
    for mutation in ("class_bottom_right", "margin_tap_no_wrap"):
        for g in ov.GEOMETRIES:
            if g.device:
                assert (ov.reference(g, mutation) == references[g.name]).all(), (mutation, g.name)


def test_geometries_draw_something_and_leave_the_rest(references):
    for g in ov.GEOMETRIES:
        changed = (references[g.name] != ov.frame_of(g)).any(-1)
        assert changed.any(), g.name
        sx, sy = ov.coords(g.M, g.H, g.W)[:2]
        reach = (sx >= 2) & (sx <= 448) & (sy >= 2) & (sy <= 448)
        if g.device:                                    # with the margin, a pixel whose source cell is outside 2..448 has no non-zero tap
            assert not (changed & ~reach).any(), g.name


def test_rectangular_coords_equal_warp_ref_on_a_square():
    g = warp_ref.BY_NAME["S_65"]
    minv = np.linalg.inv(warp_ref.homography(g.corners, g.S))
    for a, b in zip(ov.coords(minv, g.S, g.S), warp_ref.coords(minv, g.S)):
        assert (a == b).all()


# ---- sv_corners_to_m_batch ------------------------------------------------------------------------------------------------------
def test_corners_to_m_is_the_inverse_of_minv_and_maps_the_corners(sva):
    rs = np.random.RandomState(3)
    base = np.array([[500, 100], [1400, 90], [1380, 980], [480, 1000]], np.float32)
    corners = np.stack([np.round(base + rs.uniform(-60, 60, (4, 2))).astype(np.float32)[rs.permutation(4)] for _ in range(16)])
    for size, inset in ((450, 0.0), (300, 0.05)):
        m, ok = sva.Context.corners_to_m_batch(corners, size, inset)
        minv, ok2 = sva.Context.corners_to_minv_batch(corners, size, inset)
        assert m.shape == (16, 3, 3) and m.dtype == np.float64 and ok.all() and ok2.all()
        for f in range(16):
            want = np.linalg.inv(minv[f])
            want /= want[2, 2]
            assert np.abs(m[f] - want).max() <= 1e-9 * np.abs(want).max(), f
            src = warp_ref.inset_corners(warp_ref.order_points(corners[f]), inset).astype(np.float64)
            assert np.abs(warp_ref.project(m[f], src) - warp_ref.square(size)).max() < 1e-6, f


def test_corners_to_m_degenerate_quad_is_the_identity(sva):
    corners = np.zeros((3, 4, 2), np.float32)
    corners[1] = [[10, 10], [300, 12], [310, 290], [8, 300]]
    m, ok = sva.Context.corners_to_m_batch(corners)
    _, ok2 = sva.Context.corners_to_minv_batch(corners)
    assert ok.tolist() == ok2.tolist() == [False, True, False]
    assert (m[0] == np.eye(3)).all() and (m[2] == np.eye(3)).all() and not (m[1] == np.eye(3)).all()
    lib = sva._native.lib()
    assert lib.sv_corners_to_m_batch(None, 1, 450, 0.0, None, None) == -1 and b"bad argument" in lib.sv_last_error()


def test_set_overlay_glyphs_checks_the_margin_before_anything_else(sva):
    """The margin check needs no context: it comes first, so an atlas with a non-zero margin texel is refused on any machine."""
    import ctypes as C
    lib = sva._native.lib()
    for i, j in ((2, 20), (20, 2), (47, 20), (20, 49), (0, 0)):
        atlas = ov.full_atlas()
        atlas[4, i, j] = 1
        assert lib.sv_set_overlay_glyphs(None, atlas.ctypes.data_as(C.c_void_p)) == -1
        assert f"glyph 4 has a non-zero texel at row {i}, column {j}".encode() in lib.sv_last_error()
    good = ov.full_atlas()
    assert lib.sv_set_overlay_glyphs(None, good.ctypes.data_as(C.c_void_p)) == -1 and b"NULL argument" in lib.sv_last_error()


# ---- the default font --------------------------------------------------------------------------------------------------------------
def test_default_font(sva):
    from sudoku_vision_amd import overlay_font
    a = overlay_font.default_atlas()
    assert a.shape == (9, 50, 50) and a.dtype == np.uint8
    assert a.tobytes() == overlay_font.default_atlas().tobytes()
    margin = a.copy()
    margin[:, 3:47, 3:47] = 0
    assert not margin.any()
    assert len({g.tobytes() for g in a}) == 9
    for d, g in enumerate(a, 1):
        share = (g >= 128).mean()
        assert 0.05 <= share <= 0.40, (d, share)


# ---- overlay_cells -------------------------------------------------------------------------------------------------------------------
def _dropin():
    d = os.path.join(ROOT, "sudoku-vision_amd", "resolve")
    if d not in sys.path:
        sys.path.insert(0, d)
    import overlay
    assert os.path.dirname(os.path.abspath(overlay.__file__)) == d
    return overlay


def test_overlay_cells_under_both_rules(sva):
    mod = _dropin()
    rs = np.random.RandomState(11)
    sol = rs.randint(1, 10, (9, 9))
    rec = np.where(rs.uniform(size=(9, 9)) < 0.4, sol, 0)
    conf = rs.uniform(0.4, 1.0, (9, 9))
    digits, classes = mod.overlay_cells(rec.tolist(), sol.tolist())
    assert digits.dtype == classes.dtype == np.uint8 and digits.shape == classes.shape == (81,)
    assert (digits.reshape(9, 9) == np.where(rec == 0, sol, 0)).all() and not classes.any()
    digits, classes = mod.overlay_cells(rec, sol, conf, show_originals=True)
    assert (digits.reshape(9, 9) == sol).all()
    want = np.where(rec == 0, 0, np.where(conf < 0.7, 2, 1))
    assert (classes.reshape(9, 9) == want).all() and set(classes.tolist()) == {0, 1, 2}
    _, classes = mod.overlay_cells(rec, sol, None, show_originals=True)
    assert (classes.reshape(9, 9) == np.where(rec == 0, 0, 1)).all()
    _, classes = mod.overlay_cells(rec, sol, conf, show_originals=True, low_confidence=0.0)
    assert (classes.reshape(9, 9) == np.where(rec == 0, 0, 1)).all()
    unsolved = np.zeros((9, 9), int)
    assert not mod.overlay_cells(rec, unsolved)[0].any()
    with pytest.raises(ValueError):
        mod.overlay_cells(np.full((9, 9), 10), sol)
    p = mod.CellPrediction(row=1, col=2, digit=3, confidence=0.5)
    assert (p.row, p.col, p.digit, p.confidence, p.is_original) == (1, 2, 3, 0.5, True)
    preds = [mod.CellPrediction(r, c, int(rec[r, c]), float(conf[r, c]), bool(rec[r, c])) for r in range(9) for c in range(9)]
    d2, c2 = mod.cells_from_predictions(preds, sol.tolist())
    d3, c3 = mod.overlay_cells(rec, sol, conf, show_originals=True)
    assert (d2 == d3).all() and (c2 == c3).all()


# ---- legibility of the definition -----------------------------------------------------------------------------------------------------
def test_drawn_digits_can_be_told_apart(sva):
    """A fronto-parallel quad of 450 px on a grey frame: in every cell, the glyph whose own rendering (colour blended over grey by its
    coverage) is nearest in summed absolute difference to what the reference drew -- shadow included -- is the digit drawn."""
    atlas = ov.font_atlas()
    digits = (np.arange(81) % 9 + 1).astype(np.uint8)
    frame = np.full((470, 470, 3), 128, np.uint8)
    M = warp_ref.homography(warp_ref._rect(10, 10, 459, 459), 450)
    out = ov.render(frame, M, digits, None, None, atlas).astype(np.int64)
    colour = ov.DEFAULT_PALETTE[0].astype(np.int64)
    templates = [(128 * (255 - g.astype(np.int64)[..., None]) + colour * g.astype(np.int64)[..., None] + 127) // 255 for g in atlas]
    for cell in range(81):
        r, c = divmod(cell, 9)
        got = out[10 + 50 * r:60 + 50 * r, 10 + 50 * c:60 + 50 * c]
        sad = [int(np.abs(got - t).sum()) for t in templates]
        assert int(np.argmin(sad)) + 1 == digits[cell], (cell, sad)
