"""GPU: csrc/k7_preprocess_v2.hip on inputs built for the constants it tiles and accumulates by, against tests/preprocess_v2_ref.py:
exact equality over every pixel, no tolerance anywhere.  tests/test_gpu_preprocess_v2.py asks the same of noise at seven shapes;
here the contents are flat, two-level, checkered, striped or one impulse, and the shapes sit on the kernels' tile edges.  The images are
tiny on purpose.  The case lists are module-level data: tests/test_preprocess_v2_edges_ref.py imports them and shows without a GPU that
they cover what they claim and that every expected output is affordable.

The kernels' constants, by the names csrc/k7_preprocess_v2.hip gives them (G_R, CLAHE_COLS, PW_W and PW_H are literals there: the blur's
radius, the histogram loop's stride and k_pointwise's block); every shape below is written in terms of them, so a change of the tiling
shows which cases to move:
  k_box           BT output columns by BR rows per workgroup, windows up to BOX_MAX_K (a halo of BOX_MAX_K - 1 columns)
  k_morph_planes  MT pixels of a row per workgroup plus a halo of 2^levels; elements up to MORPH_MAX_K
  k_gauss21       GW by GH pixels per workgroup; the fast path needs G_R = 10 columns on either side
  k_clahe_hist    CLAHE_ROWS tile rows per workgroup, CLAHE_COLS columns per step of a row
  k_pointwise     PW_W by PW_H pixels per workgroup, one partial count per wave of PW_W columns"""
import numpy as np
import pytest
import torch

import pp2_edge_inputs as E
import preprocess_v2_ref as R
from test_gpu_preprocess_v2 import _same

pytestmark = pytest.mark.gpu

BT, BR, BOX_MAX_K = 512, 64, 1023
MT, MORPH_MAX_K = 1024, 4095
GW, GH, G_R = 64, 32, 10
CLAHE_ROWS, CLAHE_COLS = 32, 256
PW_W, PW_H = 64, 32


def ids(cases):
    return [c.id for c in cases]


def dev(ctx, img):
    return torch.from_numpy(np.ascontiguousarray(img)).to(ctx.device)


def run(ctx, c):
    """Case c on the GPU -> u8 tensor [n,H,W]."""
    d = dev(ctx, c.img)
    if c.op == "box_mean":
        return ctx.box_mean(d, *c.args)
    if c.op == "sauvola":
        return ctx.threshold_sauvola(d, *c.args)
    if c.op == "clahe":
        return ctx.clahe(d, *c.args)
    if c.op == "gauss":
        return ctx.gaussian_blur21(d)
    shape, k = c.args
    return ctx.morphology(d, E.MORPH_OPS.index(c.op), ctx.SHAPE_RECT if shape == "rect" else ctx.SHAPE_ELLIPSE, k)


def check(ctx, c):
    got, want = run(ctx, c).cpu().numpy(), E.expected(c)
    assert got.shape == want.shape
    for f, name in enumerate(c.names):
        _same(got[f], want[f], f"{c.id}: {name}")
    return got


# ---- 1. k_box: box mean -------------------------------------------------------------------------------------------------------
BOX_HEIGHTS = [BR - 1, BR, BR + 1, 2 * BR + 1]
BOX_WIDTHS = [BT - 1, BT, BT + 1]
BOX_KS = [1, 3, 97]
BOX_GEOMETRY = [(h, BOX_WIDTHS[(i + d) % 3]) for i, h in enumerate(BOX_HEIGHTS) for d in (0, 1)]       # not the full product
BOX_MAX_SHAPES = [(5, BT + 18), (BR + 6, BT + 18), (3, 5)]     # one row block; two row blocks and two column tiles, all BT + BOX_MAX_K - 1 LDS columns in use; hundreds of reflect periods


def _box_contents(shape):
    return ["noise", "checker", "two-level 0|255"], np.stack([E.noise(shape, shape[0] + shape[1]), E.checker(shape), E.two_level(shape, 0, 255, shape[1] // 2)])


def _box_max_contents(shape):
    return ["flat 255", "flat 0", "checker", "noise"], np.stack([E.flat(shape, 255), E.flat(shape, 0), E.checker(shape), E.noise(shape, 7)])


def _box_cases():
    out = []
    for shape in BOX_GEOMETRY:
        names, img = _box_contents(shape)
        out += [E.case(f"box_mean {k} {shape}", "box_mean", (k,), img, names) for k in BOX_KS]
    for shape in BOX_MAX_SHAPES:
        names, img = _box_max_contents(shape)
        out.append(E.case(f"box_mean {BOX_MAX_K} {shape}", "box_mean", (BOX_MAX_K,), img, names))
    return out


BOX_CASES = _box_cases()


@pytest.mark.parametrize("c", BOX_CASES, ids=ids(BOX_CASES))
def test_box_mean(ctx, c):
    """Row blocks of BR, column tiles of BT with their halo, and at BOX_MAX_K on a saturated frame the largest sums the kernel can meet."""
    got = check(ctx, c)
    for f, name in enumerate(c.names):
        if name.startswith("flat"):
            assert (got[f] == c.img[f]).all(), f"{c.id}: the mean of {name} is not {name}"


def test_box_window_above_the_maximum_is_refused_and_the_next_call_works(ctx):
    from sudoku_vision_amd._native import NativeError
    img = E.noise((9, 20), 3)
    d = dev(ctx, img)[None]
    with pytest.raises(NativeError, match="SV_ERR_UNSUPPORTED"):
        ctx.box_mean(d, BOX_MAX_K + 2)
    _same(ctx.box_mean(d, 5)[0], R.box_mean(img, 5), "box_mean 5 after the refusal")
    with pytest.raises(NativeError, match="SV_ERR_UNSUPPORTED"):
        ctx.threshold_sauvola(d, BOX_MAX_K + 2, 0.2)
    _same(ctx.threshold_sauvola(d, 5, 0.2)[0], R.threshold_sauvola(img, 5, 0.2), "sauvola 5 after the refusal")


# ---- 2. k_box: Sauvola --------------------------------------------------------------------------------------------------------
SAUVOLA_FLAT_WINDOWS = [1, 3, 25]
SAUVOLA_FLAT_KS = [0.0, 0.2, 0.5]
TWO_LEVEL_PAIRS = [(0, 255), (254, 255), (0, 1), (127, 128)]
TWO_LEVEL_SHAPE = (12, 40)


def _sauvola_cases():
    out = []
    for shape in BOX_GEOMETRY:
        out.append(E.case(f"sauvola 25 0.2 {shape}", "sauvola", (25, 0.2), np.stack([E.noise(shape, 11 + shape[0]), E.checker(shape)]), ["noise", "checker"]))
    for shape in BOX_MAX_SHAPES[:2]:
        img = np.stack([E.flat(shape, 255), E.checker(shape), E.noise(shape, 8)])
        out += [E.case(f"sauvola {BOX_MAX_K} {k} {shape}", "sauvola", (BOX_MAX_K, k), img, ["flat 255", "checker", "noise"]) for k in (0.2, 0.5)]
    H, W = TWO_LEVEL_SHAPE
    names = [f"{lo}|{hi} split at {s}" for lo, hi in TWO_LEVEL_PAIRS for s in (1, W // 2, W - 1)]
    img = np.stack([E.two_level(TWO_LEVEL_SHAPE, lo, hi, s) for lo, hi in TWO_LEVEL_PAIRS for s in (1, W // 2, W - 1)])
    out += [E.case(f"sauvola two-level {w} {k}", "sauvola", (w, k), img, names) for w in (3, 25) for k in (0.0, 0.2, 0.34)]
    return out


def _sauvola_flat_cases():
    img = np.stack([E.flat((5, 5), v) for v in range(256)])                  # every grey level, one flat frame each, one launch
    return [E.case(f"sauvola flat {w} {k}", "sauvola", (w, k), img, [f"flat {v}" for v in range(256)]) for w in SAUVOLA_FLAT_WINDOWS for k in SAUVOLA_FLAT_KS]


SAUVOLA_CASES = _sauvola_cases()
SAUVOLA_FLAT_CASES = _sauvola_flat_cases()


@pytest.mark.parametrize("c", SAUVOLA_CASES, ids=ids(SAUVOLA_CASES))
def test_sauvola(ctx, c):
    """The box geometry again with the squares' sums; BOX_MAX_K on a saturated frame, where only 64-bit sums of squares are right; and two-level
    images, on which sq - mean^2 cancels."""
    check(ctx, c)


@pytest.mark.parametrize("c", SAUVOLA_FLAT_CASES, ids=ids(SAUVOLA_FLAT_CASES))
def test_sauvola_flat_frames(ctx, c):
    """Variance exactly 0 at every grey level.  At k = 0 the threshold is the mean, the pixel ties with it, and a tie is not "<"."""
    got = check(ctx, c)
    if c.args[1] == 0.0:
        assert not got.any(), f"{c.id}: a flat pixel came out below its own mean"


def test_sauvola_ties(ctx):
    """3 x 3 images whose centre pixel equals its float32 threshold exactly (E.sauvola_ties, window 3).  What the search finds: at k = 0.2
    and 0.5 the all-zero image is the only tie among the 5^9 images; at k = 0 the threshold is the mean and 7,649 images tie, 5 flat and 7,644
    with positive variance whose mean is the centre value.  The first 32 are kept: the zero image at each k and 29 non-flat ones at k = 0."""
    ties = E.sauvola_ties()
    assert ties
    for k in sorted({k for _, k in ties}):
        imgs = np.stack([img for img, kk in ties if kk == k])
        got = ctx.threshold_sauvola(dev(ctx, imgs), 3, k).cpu().numpy()
        for f, img in enumerate(imgs):
            _same(got[f], R.threshold_sauvola(img, 3, k), f"sauvola tie k {k} {img.ravel().tolist()}")
            assert got[f][1, 1] == 0


# ---- 3. CLAHE -----------------------------------------------------------------------------------------------------------------
CLAHE_FLAT_LEVELS = [0, 1, 77, 254, 255]
CLAHE_FLAT_SIZES = [((2 * CLAHE_ROWS, 2 * CLAHE_COLS), (2, 2)), ((2 * CLAHE_ROWS + 2, 2 * CLAHE_COLS + 2), (2, 2)), ((CLAHE_ROWS + 1, CLAHE_COLS + 1), (1, 1)),
                    ((40, 40), (8, 8))]
CLAHE_CLIPS = [2.0, 40.0, 0.0, 0.001]                       # 0.001: clip_limit = max(0, 1) = 1
RESIDUALS = [0, 1, 2, 128, 129, 255]                        # the step 256 / residual drops to 1 at 129
RESIDUAL_TILE = (CLAHE_ROWS, 64)
# clip, m: at 2.0 the rest spreads over ~90 other values, at 40.0 over 5 (few-value), at 100.0 over one (two-value)
RESIDUAL_FILLS = [(2.0, 2), (40.0, 1), (100.0, 2)]
CLAHE_EDGE_TILES = [(th, 40) for th in (CLAHE_ROWS - 1, CLAHE_ROWS, CLAHE_ROWS + 1, 2 * CLAHE_ROWS, 2 * CLAHE_ROWS + 1)] + \
                   [(8, tw) for tw in (CLAHE_COLS - 1, CLAHE_COLS, CLAHE_COLS + 1)]


def _residual_cases():
    """-> [(case, clip, [(tile, intended residual)])]: one tile on an image of its size, and 2 x 2 tiles with four different residuals."""
    th, tw = RESIDUAL_TILE
    out = []
    for clip, m in RESIDUAL_FILLS:
        for i, r in enumerate(RESIDUALS):
            tile, r = E.clahe_residual_tile(th, tw, clip, r, m, (0, 77, 255)[i % 3], 100 + i)
            out.append((E.case(f"clahe residual {r} clip {clip} (1, 1)", "clahe", (clip, (1, 1)), tile), clip, [(tile, r)]))
    for clip, m in RESIDUAL_FILLS[:2]:
        for i in range(len(RESIDUALS)):
            four = [E.clahe_residual_tile(th, tw, clip, RESIDUALS[(i + j) % 6], m, (31 * i + 64 * j) % 256, 200 + 4 * i + j) for j in range(4)]
            img = np.block([[four[0][0], four[1][0]], [four[2][0], four[3][0]]])
            out.append((E.case(f"clahe residuals {[r for _, r in four]} clip {clip} (2, 2)", "clahe", (clip, (2, 2)), img), clip, four))
    return out


def _clahe_cases():
    out = []
    for shape, tiles in CLAHE_FLAT_SIZES:
        img = np.stack([E.flat(shape, v) for v in CLAHE_FLAT_LEVELS])
        out += [E.case(f"clahe flat {shape} {tiles} clip {clip}", "clahe", (clip, tiles), img, [f"flat {v}" for v in CLAHE_FLAT_LEVELS]) for clip in CLAHE_CLIPS]
    for th, tw in CLAHE_EDGE_TILES:
        # tiles = (tiles_x, tiles_y); the ragged size is one short of a multiple in both directions, so the reflect extension supplies a row and a column
        for tiles, short in [((1, 1), 0), ((2, 3), 0), ((2, 3), 1)]:
            shape = (tiles[1] * th - short, tiles[0] * tw - short)
            out.append(E.case(f"clahe tile {th}x{tw} {tiles} image {shape}", "clahe", (2.0, tiles), E.noise(shape, th + tw)))
    for shape, tiles in [((96, 160), (8, 8)), ((17, 33), (3, 5))]:
        img = np.stack([E.checker(shape), E.stripes_h(shape), E.stripes_v(shape)])
        out += [E.case(f"clahe extreme {shape} {tiles} clip {clip}", "clahe", (clip, tiles), img, ["checker", "stripes_h", "stripes_v"]) for clip in (2.0, 0.0)]
    return out


CLAHE_RESIDUAL_CASES = _residual_cases()
CLAHE_CASES = _clahe_cases() + [c for c, _, _ in CLAHE_RESIDUAL_CASES]


@pytest.mark.parametrize("c", CLAHE_CASES, ids=ids(CLAHE_CASES))
def test_clahe(ctx, c):
    """Flat tiles (one bin holds the area), tiles built so that the clipped total leaves each residual of RESIDUALS, tile heights about
    CLAHE_ROWS and widths about CLAHE_COLS with and without the reflect extension, and images of 0 and 255 only."""
    check(ctx, c)


# ---- 4. morphology ------------------------------------------------------------------------------------------------------------
MORPH_KS = [4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65]        # 2^l - 1, 2^l, 2^l + 1: the level changes and the two windows coincide
MORPH_KS_AT_W = [16, 17, 32, 33]
IMPULSE_KS = [2, 3, 6, 7, 33, 65]
IMPULSE_SHAPE = (40, MT + 76)
IMPULSE_AT = [(0, 0), (39, MT + 75), (20, MT - 1), (20, MT), (20, 0), (0, (MT + 76) // 2)]
SEAM_WIDTHS = [MT - 1, MT, MT + 1, MT + 32]
IDENTITY_WIDTHS = [1, 33, MT + 1]
IDENTITY_KS = [3, 51, 193]
MORPH_MAX_SHAPE = (6, MT + 76)


def _morph_size_cases():
    out = []
    for shape in ("rect", "ellipse"):
        for k in MORPH_KS:
            widths = [70] + ([k - 1, k, k + 1] if k in MORPH_KS_AT_W else [])           # W just above k; min(k, W) takes the level
            out += [E.case(f"{op} {shape} {k} on 20x{W}", op, (shape, k), E.noise((20, W), k + W)) for W in widths for op in E.MORPH_OPS]
    return out


def _impulse_cases():
    """-> [(dilate case, erode case)]: one frame per impulse position; the erode case is the dilate case inverted."""
    out = []
    for shape in ("rect", "ellipse"):
        for k in IMPULSE_KS:
            names = [f"impulse at {p}" for p in IMPULSE_AT]
            on = np.stack([E.impulse(IMPULSE_SHAPE, y, x) for y, x in IMPULSE_AT])
            off = np.stack([E.impulse(IMPULSE_SHAPE, y, x, on=0, off=255) for y, x in IMPULSE_AT])
            out.append((E.case(f"dilate {shape} {k} impulses", "dilate", (shape, k), on, names), E.case(f"erode {shape} {k} impulses", "erode", (shape, k), off, names)))
    return out


def _seam_cases():
    out = []
    for W in SEAM_WIDTHS:
        img = np.stack([E.noise((6, W), W), E.stripes_v((6, W))])
        out += [E.case(f"{op} {shape} {k} on 6x{W}", op, (shape, k), img, ["noise", "stripes_v"]) for op in ("close", "open") for shape, k in (("ellipse", 51), ("rect", 33))]
    return out


def _identity_cases():
    out = []
    for W in IDENTITY_WIDTHS:
        names, img = E.extreme((5, W))
        for shape in ("rect", "ellipse"):
            for k in IDENTITY_KS:
                out += [E.case(f"{op} {shape} {k} extreme 5x{W}", op, (shape, k), img, names) for op in E.MORPH_OPS]
    return out


def _morph_max_cases():
    """R._morph cannot afford MORPH_MAX_K (see E.morph_direct): the expected output is the definition evaluated directly."""
    img = np.stack([E.noise(MORPH_MAX_SHAPE, 5), E.impulse(MORPH_MAX_SHAPE, 2, MT + 70)])
    return [E.case(f"{op} {shape} {MORPH_MAX_K} on {MORPH_MAX_SHAPE}", op, (shape, MORPH_MAX_K), img, ["noise", "impulse"], ref="direct")
            for shape in ("rect", "ellipse") for op in ("dilate", "close")]


MORPH_SIZE_CASES = _morph_size_cases()
IMPULSE_CASES = _impulse_cases()
SEAM_CASES = _seam_cases()
IDENTITY_CASES = _identity_cases()
MORPH_MAX_CASES = _morph_max_cases()


@pytest.mark.parametrize("c", MORPH_SIZE_CASES, ids=ids(MORPH_SIZE_CASES))
def test_morphology_element_sizes_about_powers_of_two(ctx, c):
    check(ctx, c)


@pytest.mark.parametrize("pair", IMPULSE_CASES, ids=[d.id for d, _ in IMPULSE_CASES])
def test_morphology_of_an_impulse_is_the_element(ctx, pair):
    """At the image's corners, on both sides of the k_morph_planes seam at MT, and at the left and top edges.  Apart from the restatement: the
    dilated impulse is the element reflected through its anchor and clipped to the image (E.impulse_footprint), and the eroded inverse is
    its complement."""
    dilated, eroded = check(ctx, pair[0]), check(ctx, pair[1])
    el = R.structuring_element(*pair[0].args)
    for f, (y, x) in enumerate(IMPULSE_AT):
        want = E.impulse_footprint(IMPULSE_SHAPE, y, x, el)
        _same(dilated[f], want, f"{pair[0].id}: footprint at {(y, x)}")
        _same(eroded[f], 255 - want, f"{pair[1].id}: footprint at {(y, x)}")


@pytest.mark.parametrize("c", SEAM_CASES, ids=ids(SEAM_CASES))
def test_morphology_across_the_planes_tile_seam(ctx, c):
    check(ctx, c)


@pytest.mark.parametrize("c", IDENTITY_CASES, ids=ids(IDENTITY_CASES))
def test_morphology_beyond_the_edge_is_identity(ctx, c):
    """Pixels outside the image are 0 to a maximum and 255 to a minimum, so all four operations give a flat frame back unchanged: a wrong
    identity darkens the border of flat 255 under erode or lights that of flat 0 under dilate.  The checker, the third extreme frame, cannot come
    back unchanged from an element of 3 or more on 5 rows: every pixel has a vertical neighbour of the other colour, so dilate and close
    give flat 255 and erode and open flat 0, which is asserted in its place."""
    got = check(ctx, c)
    for f, name in enumerate(c.names):
        want = c.img[f] if name.startswith("flat") else E.flat(c.img[f].shape, 255 if c.op in ("dilate", "close") else 0)
        _same(got[f], want, f"{c.id}: {name}")


@pytest.mark.parametrize("c", MORPH_MAX_CASES, ids=ids(MORPH_MAX_CASES))
def test_morphology_at_the_largest_element(ctx, c):
    check(ctx, c)


# ---- 5. Gaussian --------------------------------------------------------------------------------------------------------------
GAUSS_SHAPES = [(h, w) for h in (GH - 1, GH, GH + 1) for w in (GW - 1, GW, GW + 1)] + [(12, w) for w in (G_R, G_R + 1, 2 * G_R, 2 * G_R + 1, 2 * G_R + 2)]
GAUSS_FLAT_SHAPES = [(GH + 1, GW + 1), (1, 1), (7, 1)]
GAUSS_IMPULSE = ((GH + 1, GW + 1), (GH // 2, GW // 2))


def _gauss_cases():
    out = []
    for shape in GAUSS_FLAT_SHAPES:
        out.append(E.case(f"gauss flat {shape}", "gauss", (), np.stack([E.flat(shape, v) for v in (255, 0, 1)]), ["flat 255", "flat 0", "flat 1"]))
    for shape in GAUSS_SHAPES:
        img = np.stack([E.stripes_h(shape, 1), E.stripes_v(shape, 1), E.stripes_h(shape, 2), E.stripes_v(shape, 2), E.checker(shape)])
        out.append(E.case(f"gauss patterns {shape}", "gauss", (), img, ["stripes_h 1", "stripes_v 1", "stripes_h 2", "stripes_v 2", "checker"]))
    shape, (y, x) = GAUSS_IMPULSE
    img = np.stack([E.two_level(shape, 0, 255, shape[1] // 2), np.ascontiguousarray(E.two_level(shape[::-1], 0, 255, shape[0] // 2).T), E.impulse(shape, y, x)])
    out.append(E.case(f"gauss step and impulse {shape}", "gauss", (), img, ["step across the columns", "step down the rows", f"impulse at {(y, x)}"]))
    return out


GAUSS_CASES = _gauss_cases()


@pytest.mark.parametrize("c", GAUSS_CASES, ids=ids(GAUSS_CASES))
def test_gaussian_blur21(ctx, c):
    """The taps sum to 256 and a row sum of a saturated frame is 255 * 256, the largest an unsigned short holds: a flat frame comes back as it
    went in.  Patterns of 0 and 255 on the GW x GH tile edges and on the widths where the unreflected fast path switches on."""
    got = check(ctx, c)
    for f, name in enumerate(c.names):
        if name.startswith("flat"):
            assert (got[f] == c.img[f]).all(), f"{c.id}: {name} did not come back as {name}"


# ---- 6. pointwise counts ------------------------------------------------------------------------------------------------------
COUNT_SHAPES = [(PW_H + 1, PW_W + 1), (PW_H, PW_W), (1, 1), (40, 32 * PW_W + 1)]


def _count_frames(shape):
    """flat 0, flat 255, only the last pixel set, and about half: per-frame counts 0, H W, 1 and roughly H W / 2, in one batch."""
    last = E.impulse(shape, shape[0] - 1, shape[1] - 1)
    return np.stack([E.flat(shape, 0), E.flat(shape, 255), last, np.where(E.noise(shape, 9) < 128, 0, 255).astype(np.uint8)])


@pytest.mark.parametrize("shape", COUNT_SHAPES)
def test_counts_on_all_clear_all_set_and_last_pixel_only(ctx, shape):
    """Each frame alone, then the four as one batch: every frame gets its own count."""
    frames = _count_frames(shape)
    want = np.where(frames > 127, 255, 0).astype(np.uint8)
    n = [int(np.count_nonzero(w)) for w in want]
    assert n[:3] == [0, shape[0] * shape[1], 1] and (shape == (1, 1) or 0 < n[3] < shape[0] * shape[1])
    # gray - mean < -30 exactly where the frame is set: gray is the frame inverted, the mean a flat 100 (155 against -100)
    inverted, mean = 255 - frames, np.full_like(frames, 100)
    for sel in [slice(0, 1), slice(1, 2), slice(2, 3), slice(3, 4), slice(0, 4)]:
        d, what = dev(ctx, frames[sel]), f"{shape} frames {sel.start}..{sel.stop - 1}"
        mask, cnt = ctx.threshold_count(d, 127)
        _same(mask, want[sel], f"threshold {what}")
        assert cnt.tolist() == n[sel], f"threshold count {what}"
        mask, cnt = ctx.threshold_count(d, 127, inv=True)
        _same(mask, 255 - want[sel], f"threshold inv {what}")
        assert cnt.tolist() == [shape[0] * shape[1] - v for v in n[sel]], f"threshold inv count {what}"
        mask, cnt = ctx.shadow_mask(dev(ctx, inverted[sel]), dev(ctx, mean[sel]))
        _same(mask, want[sel], f"shadow mask {what}")
        assert cnt.tolist() == n[sel], f"shadow count {what}"
        assert ctx.count_nonzero(d).tolist() == n[sel], f"count_nonzero {what}"


@pytest.mark.parametrize("shape", COUNT_SHAPES)
def test_divide_by_flat_backgrounds(ctx, shape):
    """A background of 0 counts as 1, so every gray above 0 saturates; a background of 255 gives the gray back."""
    names, gray = E.extreme(shape)
    for b in (0, 255):
        back = np.full_like(gray, b)
        got = ctx.divide_normalize(dev(ctx, gray), dev(ctx, back)).cpu().numpy()
        for f, name in enumerate(names):
            _same(got[f], R.divide_normalize(gray[f], back[f]), f"divide {name} by flat {b} {shape}")
            _same(got[f], gray[f], f"divide {name} by flat {b} {shape}: extreme gray comes back")


# ---- 7. scratch order ---------------------------------------------------------------------------------------------------------
SCRATCH_CASES = [E.case("scratch: close ellipse 193 on 130x700", "close", ("ellipse", 193), E.noise((130, 700), 1)),
                 E.case("scratch: clahe (8, 8) on 40x40", "clahe", (2.0, (8, 8)), E.noise((40, 40), 2)),
                 E.case("scratch: dilate rect 3 on 5x5", "dilate", ("rect", 3), E.noise((5, 5), 3)),
                 E.case("scratch: clahe (3, 5) on 96x160", "clahe", (2.0, (3, 5)), E.noise((96, 160), 4)),
                 E.case("scratch: open rect 2 on 130x700", "open", ("rect", 2), E.noise((130, 700), 5))]


@pytest.mark.parametrize("order", [1, -1], ids=["forward", "reverse"])
def test_scratch_shared_by_morphology_and_clahe(order):
    """sv_ctx::pp2 holds the element rows, planes and intermediate of a morphology call or the histograms and LUTs of a CLAHE call, at different
    layouts in one grow-only buffer.  On a context of its own, large and small calls of both kinds alternate: each must write whatever it reads."""
    import sudoku_vision_amd as sva
    c = sva.Context()
    try:
        for case in SCRATCH_CASES[::order]:
            check(c, case)
    finally:
        c.close()


ALL_CASES = BOX_CASES + SAUVOLA_CASES + SAUVOLA_FLAT_CASES + CLAHE_CASES + MORPH_SIZE_CASES + [c for pair in IMPULSE_CASES for c in pair] + SEAM_CASES + \
            IDENTITY_CASES + MORPH_MAX_CASES + GAUSS_CASES + SCRATCH_CASES
