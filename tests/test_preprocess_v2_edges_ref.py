"""The CPU half of tests/test_gpu_preprocess_v2_edges.py: that module's case lists are data, and this one shows without a GPU that they
cover what they claim (the box geometry, the CLAHE residuals), that what the GPU tests assert besides equality with the restatement
agrees with the restatement (the impulse footprint, flat frames coming back, the Sauvola ties), that the direct morphology used at the
largest element is the restatement's, and that every expected output can be computed within the time cap."""
import time

import numpy as np
import pytest

import pp2_edge_inputs as E
import preprocess_v2_ref as R
import test_gpu_preprocess_v2_edges as G

SECONDS_PER_CASE = 5.0


# ---- 1: geometry ------------------------------------------------------------------------------------------------------------
def test_box_geometry_covers_the_issue():
    assert (G.BT, G.BR, G.BOX_MAX_K) == (512, 64, 1023)
    assert G.BOX_HEIGHTS == [63, 64, 65, 129] and G.BOX_WIDTHS == [511, 512, 513] and G.BOX_KS == [1, 3, 97]
    for h in G.BOX_HEIGHTS:
        assert len({w for hh, w in G.BOX_GEOMETRY if hh == h}) >= 2
    for w in G.BOX_WIDTHS:
        assert len({h for h, ww in G.BOX_GEOMETRY if ww == w}) >= 2
    ran = {(c.img.shape[1:], c.args[0]) for c in G.BOX_CASES}
    for h in G.BOX_HEIGHTS:
        for k in G.BOX_KS:
            assert any(shape[0] == h and kk == k for shape, kk in ran), (h, k)
    assert {(shape, G.BOX_MAX_K) for shape in [(5, 530), (70, 530), (3, 5)]} <= ran
    assert {c.img.shape[1:] for c in G.SAUVOLA_CASES if c.id.startswith("sauvola 25 0.2")} == set(G.BOX_GEOMETRY)
    two = [c for c in G.SAUVOLA_CASES if c.id.startswith("sauvola two-level")]
    assert {c.args for c in two} == {(w, k) for w in (3, 25) for k in (0.0, 0.2, 0.34)} and all(c.img.shape == (12, 12, 40) for c in two)
    assert {(c.img.shape[1:], c.args) for c in G.SAUVOLA_CASES if c.args[0] == G.BOX_MAX_K} == {(s, (1023, k)) for s in [(5, 530), (70, 530)] for k in (0.2, 0.5)}


def test_case_ids_are_unique():
    ids = [c.id for c in G.ALL_CASES]
    assert len(set(ids)) == len(ids)


# ---- 3: CLAHE residuals -------------------------------------------------------------------------------------------------------
def test_clahe_tiles_leave_the_residuals_they_aim_at():
    """From each tile's histogram in plain numpy; and the restatement's own redistribution is what these tiles reach: `a` alone is clipped."""
    single, quads = set(), set()
    for c, clip, tiles in G.CLAHE_RESIDUAL_CASES:
        th, tw = G.RESIDUAL_TILE
        assert c.img.shape[1:] == (th * c.args[1][1], tw * c.args[1][0]) and c.args[0] == clip
        for t, (tile, r) in enumerate(tiles):
            ty, tx = divmod(t, c.args[1][0])
            assert (c.img[0, ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw] == tile).all()
            hist = np.bincount(tile.ravel(), minlength=256)
            limit = max(int(clip * tile.size / 256), 1)
            assert int(np.maximum(hist - limit, 0).sum()) % 256 == r == E.clahe_residual(tile, clip)
            assert np.count_nonzero(hist > limit) == 1
            (single if len(tiles) == 1 else quads).add(r)
        if len(tiles) == 4:
            assert len({r for _, r in tiles}) == 4
    assert single == quads == set(G.RESIDUALS) == {0, 1, 2, 128, 129, 255}
    values = {clip: {np.count_nonzero(np.bincount(tiles[0][0].ravel())) for _, cl, tiles in G.CLAHE_RESIDUAL_CASES if cl == clip and len(tiles) == 1} for clip, _ in G.RESIDUAL_FILLS}
    assert values[100.0] == {2} and max(values[40.0]) <= 6 and min(values[2.0]) > 50          # two-value, few-value, many-value


def test_clahe_sizes_cover_the_issue():
    flat = {(c.img.shape[1:], c.args[1], c.args[0]) for c in G.CLAHE_CASES if c.id.startswith("clahe flat")}
    assert flat == {(s, t, clip) for s, t in [((64, 512), (2, 2)), ((66, 514), (2, 2)), ((33, 257), (1, 1)), ((40, 40), (8, 8))] for clip in (2.0, 40.0, 0.0, 0.001)}
    assert E.clahe_clip_limit(0.001, 32 * 256) == 1 and E.clahe_clip_limit(0.0, 32 * 256) == 0
    tiles, ragged = set(), 0
    for c in G.CLAHE_CASES:
        if c.id.startswith("clahe tile"):
            (H, W), (tx, ty) = c.img.shape[1:], c.args[1]
            ext = R.clahe_extend(c.img[0], tx, ty)
            tiles.add((ext.shape[0] // ty, ext.shape[1] // tx, (tx, ty)))
            ragged += ext.shape != (H, W)
    assert tiles == {(th, tw, g) for th, tw in [(31, 40), (32, 40), (33, 40), (64, 40), (65, 40), (8, 255), (8, 256), (8, 257)] for g in [(1, 1), (2, 3)]}
    assert ragged == 8


# ---- 2: Sauvola ties and flat frames ------------------------------------------------------------------------------------------
def test_sauvola_tie_search():
    ties = E.sauvola_ties()
    assert 0 < len(ties) <= E.TIE_KEEP
    again = E.sauvola_ties()
    assert len(again) == len(ties) and all((a[0] == b[0]).all() and a[1] == b[1] for a, b in zip(ties, again))
    for img, k in ties:
        assert img.shape == (3, 3) and img.dtype == np.uint8 and set(img.ravel()) <= set(E.TIE_LEVELS) and k in E.TIE_KS
        s1, s2 = int(img.astype(np.int64).sum()), int((img.astype(np.int64) ** 2).sum())
        assert R.window_sums(img, 3)[1, 1] == s1 and R.window_sums(img, 3, square=True)[1, 1] == s2
        assert np.float32(img[1, 1]) == R.sauvola_threshold_from_sums(np.array([s1]), np.array([s2]), 3, k)[0]
        assert R.threshold_sauvola(img, 3, k)[1, 1] == 0                      # a tie is not "<"
    # what the GPU test's docstring says the search finds
    assert [(img.ravel().tolist(), k) for img, k in ties[:3]] == [([0] * 9, 0.0), ([0] * 9, 0.2), ([0] * 9, 0.5)]
    assert all(k == 0.0 and len(set(img.ravel())) > 1 for img, k in ties[3:]) and len(ties) == 32


def test_sauvola_flat_frames_at_k0_are_all_clear():
    for c in G.SAUVOLA_FLAT_CASES:
        assert c.img.shape == (256, 5, 5) and [int(f[0, 0]) for f in c.img] == list(range(256)) and all((f == f[0, 0]).all() for f in c.img)
        if c.args[1] == 0.0:
            assert not E.expected(c).any()
    assert {c.args for c in G.SAUVOLA_FLAT_CASES} == {(w, k) for w in (1, 3, 25) for k in (0.0, 0.2, 0.5)}


# ---- 4: morphology ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", [("rect", 2), ("rect", 3), ("ellipse", 6), ("ellipse", 7), ("rect", 33), ("ellipse", 33), ("ellipse", 65)])
def test_impulse_footprint_is_what_the_restatement_dilates_to(shape, k):
    el = R.structuring_element(shape, k)
    size = (40, 90)
    for y, x in [(0, 0), (39, 89), (20, 45), (20, 0), (0, 45), (1, 88)]:
        want = E.impulse_footprint(size, y, x, el)
        assert (R.dilate(E.impulse(size, y, x), el) == want).all(), (y, x)
        assert (R.erode(E.impulse(size, y, x, on=0, off=255), el) == 255 - want).all(), (y, x)
    at = 2 * k - 1 - k // 2                                                      # element cell (i, j) lands on (2k - 1 - i, 2k - 1 - j)
    inside = E.impulse_footprint((3 * k, 3 * k), at, at, el)                     # nothing clipped: the element itself, reflected
    assert (inside[k:2 * k, k:2 * k] == 255 * el[::-1, ::-1]).all() and inside.sum() == 255 * el.sum()


def test_impulse_cases_cover_the_issue():
    assert G.IMPULSE_SHAPE == (40, 1100) and G.IMPULSE_AT == [(0, 0), (39, 1099), (20, 1023), (20, 1024), (20, 0), (0, 550)]
    assert {d.args for d, _ in G.IMPULSE_CASES} == {(s, k) for s in ("rect", "ellipse") for k in (2, 3, 6, 7, 33, 65)}
    for d, e in G.IMPULSE_CASES:
        assert (d.op, e.op) == ("dilate", "erode") and d.args == e.args and (e.img == 255 - d.img).all()
        assert [np.argwhere(f).tolist() for f in d.img] == [[list(p)] for p in G.IMPULSE_AT]


@pytest.mark.parametrize("shape,k,size", [("rect", 2, (5, 9)), ("ellipse", 7, (6, 40)), ("ellipse", 65, (6, 100)), ("rect", 33, (3, 70)), ("ellipse", 193, (4, 150)),
                                          ("rect", 193, (6, 150))])
def test_morph_direct_is_the_restatement(shape, k, size):
    el = R.structuring_element(shape, k)
    for img in (E.noise(size, k), E.impulse(size, size[0] // 2, size[1] - 3), E.checker(size)):
        for op, fn in zip(E.MORPH_OPS, (R.dilate, R.erode, R.morph_close, R.morph_open)):
            assert (E.morph_direct(img, el, op) == fn(img, el)).all(), op


def test_morph_direct_is_the_restatement_at_the_largest_rect():
    """One row span, so R._morph slides once over its padding and can be afforded: the whole image lies under the element, every output
    pixel is the frame's maximum."""
    img = E.noise((2, 40), 1)
    el = R.structuring_element("rect", G.MORPH_MAX_K)
    want = R.dilate(img, el)
    assert (E.morph_direct(img, el, "dilate") == want).all() and (want == img.max()).all()


def test_identity_cases_expect_what_the_gpu_test_asserts():
    assert {c.img.shape[1:] for c in G.IDENTITY_CASES} == {(5, 1), (5, 33), (5, 1025)}
    assert {c.args for c in G.IDENTITY_CASES} == {(s, k) for s in ("rect", "ellipse") for k in (3, 51, 193)}
    for c in G.IDENTITY_CASES:
        want = E.expected(c)
        assert c.names == ["flat 0", "flat 255", "checker"]
        assert (want[0] == 0).all() and (want[1] == 255).all() and (want[2] == (255 if c.op in ("dilate", "close") else 0)).all(), c.id


# ---- 1, 5: flat frames come back ------------------------------------------------------------------------------------------------
def test_flat_frames_come_back_from_the_mean_and_the_blur():
    seen = 0
    for c in G.BOX_CASES + G.GAUSS_CASES:
        for f, name in enumerate(c.names):
            if name.startswith("flat"):
                assert (E.expected(c)[f] == c.img[f]).all(), (c.id, name)
                seen += 1
    assert seen == 2 * 3 + 3 * 3
    assert {c.img.shape[1:] for c in G.GAUSS_CASES} >= {(h, w) for h in (31, 32, 33) for w in (63, 64, 65)} | {(12, w) for w in (10, 11, 20, 21, 22)} | {(1, 1), (7, 1)}


# ---- every expected output, within the cap --------------------------------------------------------------------------------------
def test_every_expected_output_is_affordable():
    slow = []
    for c in G.ALL_CASES:
        t0 = time.perf_counter()
        want = E.expected(c)
        dt = time.perf_counter() - t0
        assert want.shape == c.img.shape and want.dtype == np.uint8
        if dt > SECONDS_PER_CASE:
            slow.append((c.id, round(dt, 2)))
    assert not slow, slow
