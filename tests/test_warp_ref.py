"""CPU: tests/warp_ref.py (an independent numpy restatement of the warp family) against the C oracle over warp_ref.GEOMETRIES,
the exact-answer geometries against their closed forms, the oracle against the continuous per-pixel bound, the product's host
homography against the oracle and an independent DLT, and a mutation check: every rule warp_ref restates is exercised by the
geometry set (a mutated rule changes at least one output)."""
import numpy as np
import pytest

import quality_ref
import sv_oracle as o
import warp_ref as R

CORNER_GEOMS = [g for g in R.GEOMETRIES if g.corners is not None]
IDENTITY = np.eye(3)


def minv_of(g, S=None):
    """The destination -> source map of geometry g (the oracle's, which tests/test_abi.py and the test below hold bit-exact
    with the product's); identity for a degenerate quad, as corners_to_minv_batch gives."""
    S = g.S if S is None else S
    if g.minv is not None:
        return g.minv
    if g.degenerate:
        return IDENTITY
    return o.corners_to_minv(g.corners, S, g.inset)


def binary_of(g):
    """A sparse {0, 255} image of geometry g (about 1 pixel in 6 is ink)."""
    return np.where(R.frame(g, 1) < 43, 255, 0).astype(np.uint8)


@pytest.mark.parametrize("g", R.GEOMETRIES, ids=lambda g: g.name)
def test_warp_bit_exact_with_oracle(g):
    M = minv_of(g)
    for ch in (3, 1):
        img = R.frame(g, ch)
        got = R.warp(img, M, g.S)
        assert (got == o.warp_perspective_minv(img, M, g.S)).all(), (g.name, ch)
        if g.corners is not None and not g.degenerate:
            assert (got == o.warp_perspective(img, g.corners, g.S, g.inset)).all(), (g.name, ch)


@pytest.mark.parametrize("g", R.GEOMETRIES, ids=lambda g: g.name)
def test_cells_and_bands_bit_exact_with_oracle(g):
    M = minv_of(g, 450)
    img = R.frame(g, 3)
    cells = R.cells(img, M)
    assert cells.shape == (81, 28, 28)
    if g.corners is not None and not g.degenerate and g.inset == 0:
        assert (cells == o.warp_cells(img, g.corners)).all(), g.name
    assert (cells == o.extract_cells(o.warp_perspective_minv(img, M, 450))).all(), g.name
    binary = binary_of(g)
    counts = R.band_counts(binary, M)
    if g.corners is not None and not g.degenerate and g.inset == 0:
        assert (counts == quality_ref.coverage_counts(binary, g.corners)).all(), g.name
    assert (counts == quality_ref.warped_counts(o.warp_perspective_minv(binary, M, 450))).all(), g.name


@pytest.mark.parametrize("g", [g for g in R.GEOMETRIES if g.exact], ids=lambda g: g.name)
def test_exact_geometries_equal_their_closed_form(g):
    M = minv_of(g)
    for ch in (3, 1):
        img = R.frame(g, ch)
        want = R.closed_form(g, img)
        assert want.shape[:2] == (g.S, g.S)
        assert (R.warp(img, M, g.S) == want).all(), (g.name, ch)
        assert (o.warp_perspective_minv(img, M, g.S) == want).all(), (g.name, ch)


def test_half_pixel_geometry_samples_at_a_b_16():
    g = R.BY_NAME["half_pixel"]
    sx, sy, a, b, _, _ = R.coords(minv_of(g), g.S)
    assert (a == 16).all() and (b == 16).all()
    assert (sx == np.arange(g.S)[None, :]).all() and (sy == np.arange(g.S)[:, None]).all()


def test_special_paths_are_taken():
    """The geometries reach the rules they are named for."""
    g = R.BY_NAME["w_zero"]
    M = g.minv
    sx, sy, a, b, X, Y = R.coords(M, g.S)
    W = (M[2, 0] * np.arange(g.S) + M[2, 2])
    assert W[16] == 0 and (X[:, 16] == 0).all() and (Y[:, 16] == 0).all()          # W := 0 reads source pixel (0, 0)
    img = R.frame(g, 3)
    assert (R.warp(img, M, g.S)[:, 16] == img[0, 0]).all()
    assert (o.warp_perspective_minv(img, M, g.S)[:, 16] == img[0, 0]).all()
    for name in ("huge_out", "wide_sat"):
        g = R.BY_NAME[name]
        sx = R.coords(minv_of(g), g.S)[0]
        assert (sx == 32767).any() or (sx == -32768).any(), name
    g = R.BY_NAME["wide_sat"]
    sx, sy = R.coords(minv_of(g), g.S)[:2]
    assert ((sx == 32767) & (sy >= 0) & (sy < g.H - 1)).any()                     # saturated onto a column inside the image
    for name in ("edge_exact", "edge_half", "edge_scale"):
        g = R.BY_NAME[name]
        sx, sy, a, b, _, _ = R.coords(minv_of(g), g.S)
        assert (sx == g.W - 1).any() and (sy == g.H - 1).any(), name
    assert (R.coords(minv_of(R.BY_NAME["edge_half"]), 64)[2][:, -1] == 16).all()
    assert (R.warp(R.frame(R.BY_NAME["wholly_out"]), minv_of(R.BY_NAME["wholly_out"]), 64) == 0).all()


SMOOTH_EXCLUDED = {
    "wide_sat": "int16 saturation moves every sample to column 32767, far from the exact coordinate",
    "w_zero": "W := 0 at dx = 16 and W < 0 beyond: not a bilinear sample of the exact point",
}


@pytest.mark.parametrize("g", [g for g in R.GEOMETRIES if g.name not in SMOOTH_EXCLUDED], ids=lambda g: g.name)
def test_oracle_within_continuous_per_pixel_bound(g):
    """Every output pixel of the oracle within 0.5 + (|dI_x| + |dI_y|)_max / 64 + 1/32768 of float64 bilinear interpolation at
    the exact source coordinate (derivation: warp_ref.warp_continuous)."""
    M = minv_of(g)
    img = R.frame(g, 3, smooth=True)
    val, bound = R.warp_continuous(img, M, g.S)
    d = np.abs(o.warp_perspective_minv(img, M, g.S).astype(np.float64) - val)
    bad = np.argwhere(d > bound)
    assert bad.size == 0, (g.name, bad[:3].tolist(), d[tuple(bad[0])], bound[tuple(bad[0])])


def test_continuous_bound_is_tight_enough_to_matter():
    """A 1/32-px error (one unit of a or b) in the discrete warp breaks the bound somewhere on a smooth image: the bound is not
    vacuous."""
    g = R.BY_NAME["rot_30"]
    M = minv_of(g)
    img = R.frame(g, 3, smooth=True)
    val, bound = R.warp_continuous(img, M, g.S)
    sx, sy, a, b, X, _ = R.coords(M, g.S)
    X = X + 1
    off = R.sample(img, X >> 5, sy, X & 31, b)
    assert (np.abs(off.astype(np.float64) - val) > bound).any()


PRODUCT_S = (9, 16, 17, 63, 64, 65, 300, 450, 1000)


@pytest.fixture(scope="module")
def product():
    import __graft_entry__ as ge
    import sudoku_vision_amd as sva
    if not __import__("os").path.exists(sva._native.LIB_PATH):
        ge.build()
    return sva.Context


@pytest.mark.parametrize("inset", [0.0, 0.05])
def test_product_corners_to_minv_bit_exact_and_maps_the_corners(product, inset):
    good = [g for g in CORNER_GEOMS if not g.degenerate]
    corners = np.stack([g.corners for g in good])
    for S in PRODUCT_S:
        got = product.corners_to_minv(corners, S, inset)
        gotb, ok = product.corners_to_minv_batch(corners, S, inset)
        assert ok.all() and (gotb == got).all()
        for g, M in zip(good, got):
            assert (M == o.corners_to_minv(g.corners, S, inset)).all(), (g.name, S)      # bit-exact fp64
            Href = R.homography(g.corners, S, inset)
            # Minv sends the destination square's corners to the (ordered, inset) source corners ...
            src = R.inset_corners(R.order_points(g.corners), inset).astype(np.float64)
            scale = max(1.0, np.abs(src).max())
            assert np.abs(R.project(M, R.square(S)) - src).max() <= 1e-9 * scale, (g.name, S)
            # ... and is the inverse of the independent DLT's homography up to scale
            P = M @ Href
            assert np.abs(P / P[2, 2] - np.eye(3)).max() <= 1e-9 * max(1.0, np.abs(Href).max() * np.abs(M / M[2, 2]).max()), (g.name, S)


def test_order_points_ties_follow_numpy_first_index(product):
    """The product's order_points breaks ties like numpy's argmin / argmax (first index), for every input order of a quad with
    ties in x+y and y-x; an exact diamond orders to a degenerate quad: SV_ERR_DEGENERATE, ok=False and the identity."""
    import itertools
    import sudoku_vision_amd as sva
    tie = R.BY_NAME["tie_order"].corners
    for perm in itertools.permutations(range(4)):
        c = tie[list(perm)]
        try:
            Href = R.homography(c, 64)
        except ValueError:
            _, ok = product.corners_to_minv_batch(c[None], 64)
            assert not ok[0], perm
            continue
        M = product.corners_to_minv(c[None], 64)[0]
        assert (M == o.corners_to_minv(c, 64)).all(), perm
        assert np.abs(R.project(M, R.square(64)) - R.order_points(c)).max() <= 1e-9 * 110, perm
        P = M @ Href
        assert np.abs(P / P[2, 2] - np.eye(3)).max() <= 1e-9, perm
    d = R.BY_NAME["diamond"].corners
    with pytest.raises(ValueError):
        R.homography(d, 64)
    with pytest.raises(sva._native.NativeError) as e:
        product.corners_to_minv(d[None], 64)
    assert "DEGENERATE" in str(e.value).upper()
    good = R.BY_NAME["rot_30"].corners
    minv, ok = product.corners_to_minv_batch(np.stack([good, d, good]), 450)
    assert ok.tolist() == [True, False, True]
    assert (minv[1] == np.eye(3)).all() and (minv[0] == o.corners_to_minv(good, 450)).all()


RESIZE_CASES = [((56, 56), (28, 28)), ((28, 28), (56, 56)), ((40, 40), (28, 28)), ((1, 1), (28, 28)), ((28, 28), (1, 1)),
                ((3, 3), (1000, 1000)), ((37, 90), (28, 45)), ((89, 89), (28, 28)), ((5, 300), (17, 7))]


@pytest.mark.parametrize("src,dst", RESIZE_CASES, ids=lambda v: "x".join(map(str, v)))
def test_resize_bit_exact_with_oracle(src, dst):
    img = np.random.RandomState(src[0] * 1000 + dst[1]).randint(0, 256, src, dtype=np.uint8)
    want = o.resize_linear(img, (dst[1], dst[0]))
    assert (R.resize(img, (dst[1], dst[0])) == want).all()


def test_resize_half_is_the_2x2_mean():
    img = np.random.RandomState(3).randint(0, 256, (56, 56)).astype(np.int64)
    want = (img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2] + 2) >> 2
    assert (R.resize(img.astype(np.uint8), (28, 28)) == want).all()


def test_geometry_set_catches_every_mutation():
    """In the style of test_pair_tolerance_catches_mutations: each rule of warp_ref, broken on purpose, changes at least one
    output over GEOMETRIES (the warp at S, else the 81 cells or the 20 band counts; the resize cases for the resize rule), so a
    kernel that broke it would fail the GPU suite, which compares the same outputs bit for bit.  Every listed mutation is
    reachable.  The block-origin rules and half-to-even rounding change a x32 coordinate only next to a rounding tie: slow
    upsampling (tiny_40, edge_scale) meets such ties, and the tie_* geometries are built to sit on one.  The int16 saturation
    only matters where column 32767 is inside the image: the 40000-px strip wide_sat."""
    left, caught = list(R.WARP_MUTATIONS), {}
    for g in R.GEOMETRIES:
        M, img = minv_of(g), R.frame(g, 3)
        base = R.warp(img, M, g.S)
        for m in list(left):
            if (R.warp(img, M, g.S, m) != base).any():
                caught[m] = g.name
                left.remove(m)
        if not left:
            break
    for m in list(left):                        # not visible in any warp at S: the cells and band counts at 450
        for g in R.GEOMETRIES:
            M, img, binary = minv_of(g, 450), R.frame(g, 3), binary_of(g)
            if (R.cells(img, M, m) != R.cells(img, M)).any() or (R.band_counts(binary, M, m) != R.band_counts(binary, M)).any():
                caught[m] = g.name
                break
    for src, dst in RESIZE_CASES:
        img = np.random.RandomState(src[0] * 1000 + dst[1]).randint(0, 256, src, dtype=np.uint8)
        if (R.resize(img, (dst[1], dst[0])) != R.resize(img, (dst[1], dst[0]), "resize_trunc")).any():
            caught["resize_trunc"] = f"resize {src}->{dst}"
            break
    missed = sorted(set(R.MUTATIONS) - set(caught))
    assert not missed, f"mutations no geometry notices: {missed}"
    for name in ("tie_half", "tie_origin", "tie_block32"):      # the hand-built probes reach their rule on their own
        g = R.BY_NAME[name]
        m = {"tie_half": "half_away", "tie_origin": "per_pixel_origin", "tie_block32": "block_w_32"}[name]
        assert (R.warp(R.frame(g, 3), g.minv, g.S, m) != R.warp(R.frame(g, 3), g.minv, g.S)).any(), name
