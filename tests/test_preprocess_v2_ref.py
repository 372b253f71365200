"""tests/preprocess_v2_ref.py (the numpy restatement the GPU tests of cv/preprocess_v2.py compare against) held from the other
side: scipy.ndimage, the C oracle and exact rational arithmetic; the pinned constants; and the host-side decisions of the
drop-in module, which need no GPU."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage as ndi

import preprocess_v2_ref as R
import sv_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CV_DIR = os.path.join(ROOT, "sudoku-vision_amd", "cv")

NAMES = ("PreprocessResult", "grayscale", "normalize_illumination", "detect_glare", "detect_shadow", "remove_shadow", "apply_clahe",
         "threshold_adaptive", "threshold_otsu", "threshold_sauvola", "morphological_cleanup", "preprocess_for_grid_detection",
         "preprocess_multi_strategy", "preprocess_cell")

ELLIPSE_51 = [0, 7, 10, 12, 14, 15, 16, 17, 18, 19, 20, 21, 21, 22, 22, 23, 23, 24, 24, 24, 24, 25, 25, 25, 25, 25, 25, 25, 25, 25,
              24, 24, 24, 24, 23, 23, 22, 22, 21, 21, 20, 19, 18, 17, 16, 15, 14, 12, 10, 7, 0]
TAPS_21 = [0, 2, 2, 4, 6, 11, 15, 20, 25, 28, 30, 28, 25, 20, 15, 11, 6, 4, 2, 2, 0]


def _module():
    if CV_DIR not in sys.path:
        sys.path.insert(0, CV_DIR)
    import preprocess_v2
    return preprocess_v2


def _img(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


# ---- pinned constants ---------------------------------------------------------------------------------------------------------
def test_ellipse_rows_pinned():
    assert R.ellipse_half_widths(7) == [0, 2, 3, 3, 3, 2, 0]
    assert R.ellipse_half_widths(51) == ELLIPSE_51
    assert R.ellipse_half_widths(1) == [0]
    el = R.structuring_element("ellipse", 7)
    assert el.sum(1).tolist() == [1, 5, 7, 7, 7, 5, 1] and (el == el[::-1, ::-1]).all()
    assert R.structuring_element("rect", 2).tolist() == [[1, 1], [1, 1]]


def test_gauss21_taps_pinned():
    assert R.GAUSS21_SIGMA == 3.5
    assert R.gauss21_taps() == TAPS_21 and sum(TAPS_21) == 256


def test_kernel_sizes():
    assert R.illumination_kernel_size((1080, 1920)) == 193 and R.shadow_kernel_size((1080, 1920)) == 97
    assert R.illumination_kernel_size((2736, 3648)) == 365 and R.shadow_kernel_size((2736, 3648)) == 183
    assert R.illumination_kernel_size((100, 80)) == 51 and R.shadow_kernel_size((100, 80)) == 5
    assert R.shadow_kernel_size((7, 1)) == 1


# ---- morphology against scipy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 2), (13, 17), (9, 40), (33, 5)])
@pytest.mark.parametrize("element", [("rect", 1), ("rect", 2), ("rect", 3), ("rect", 4), ("ellipse", 6), ("ellipse", 7), ("ellipse", 51)])
def test_dilate_erode_equal_scipy(shape, element):
    """k up to beyond the image size; the even anchor is (k//2, k//2) with the element unreflected.  grey_dilation mirrors its
    footprint and moves an even footprint's centre, hence the mirrored footprint and origin -1 for even k."""
    img = _img(shape, 7 + shape[0] * 31 + shape[1])
    el = R.structuring_element(*element)
    even = element[1] % 2 == 0
    d = ndi.grey_dilation(img, footprint=el[::-1, ::-1], mode="constant", cval=0, origin=-1 if even else 0)
    e = ndi.grey_erosion(img, footprint=el, mode="constant", cval=255)
    assert (R.dilate(img, el) == d).all()
    assert (R.erode(img, el) == e).all()
    assert (d == ndi.maximum_filter(img, footprint=el, mode="constant", cval=0)).all()      # the same statement without the mirroring
    assert (R.morph_close(img, el) == ndi.grey_erosion(d, footprint=el, mode="constant", cval=255)).all()
    assert (R.morph_open(img, el) == ndi.grey_dilation(e, footprint=el[::-1, ::-1], mode="constant", cval=0, origin=-1 if even else 0)).all()


def test_open_2x2_is_shifted_not_symmetric():
    img = np.zeros((6, 6), np.uint8)
    img[2:4, 2:4] = 255
    el = R.structuring_element("rect", 2)
    assert np.argwhere(R.erode(img, el)).tolist() == [[3, 3]]                # offsets {-1, 0}: only the lower right pixel survives
    want = np.zeros((6, 6), np.uint8)
    want[3:5, 3:5] = 255                                                       # both passes use the element unreflected: the block moves by one
    assert (R.morph_open(img, el) == want).all()


# ---- box mean, Gaussian ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", [((1, 1), 3), ((1, 7), 5), ((7, 1), 5), ((2, 2), 7), ((17, 33), 9), ((40, 60), 21), ((5, 9), 31)])
def test_box_mean_equals_rounded_exact_mean(shape, k):
    img = _img(shape, 100 + k)
    exact = ndi.uniform_filter(img.astype(np.float64), k, mode="mirror")
    clear = np.abs(exact - np.floor(exact) - 0.5) > 1e-6
    assert clear.any()
    assert (R.box_mean(img, k)[clear] == np.rint(exact)[clear]).all()


def test_reflect101_index():
    assert R.reflect101_index(np.arange(-7, 9), 4).tolist() == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert R.reflect101_index(np.arange(-3, 4), 1).tolist() == [0] * 7


@pytest.mark.parametrize("shape", [(200, 300), (5, 64), (64, 5), (1, 1)])
def test_gaussian_blur21_within_2_of_float(shape):
    img = _img(shape, 5)
    ref = ndi.gaussian_filter(img.astype(np.float64), 3.5, mode="mirror", radius=10)
    dev = np.abs(R.gaussian_blur21(img).astype(np.float64) - ref)
    assert dev.max() <= 2.0, f"max deviation {dev.max():.3f}; share of pixels beyond 1: {(dev > 1).mean():.5f}"


def test_divide_normalize():
    g = np.array([[0, 10, 200, 255, 255, 7]], np.uint8)
    b = np.array([[0, 20, 100, 255, 1, 9]], np.uint8)
    want = [0, 127, 255, 255, 255, int(np.float32(7) / np.float32(9) * np.float32(255))]
    assert R.divide_normalize(g, b).tolist() == [want]


# ---- CLAHE, Otsu against the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,tiles,clip", [((64, 64), (8, 8), 2.0), ((28, 28), (4, 4), 2.0), ((96, 160), (8, 8), 2.0), ((48, 40), (4, 8), 40.0),
                                              ((32, 32), (8, 8), 0.0)])
def test_clahe_equals_oracle_on_divisible_sizes(shape, tiles, clip):
    img = (_img(shape, 11) // 3 + np.arange(shape[1], dtype=np.uint8)[None, :] // 2).astype(np.uint8)
    assert (R.clahe(img, clip, tiles) == sv_oracle.clahe(img, clip, tiles)).all()


@pytest.mark.parametrize("shape,tiles", [((30, 45), (4, 4)), ((17, 33), (8, 8)), ((1, 7), (8, 8)), ((7, 1), (4, 4)), ((1, 1), (8, 8)), ((2, 2), (8, 8)),
                                         ((100, 64), (8, 8))])
def test_clahe_on_other_sizes_is_the_oracle_on_the_extended_image(shape, tiles):
    img = _img(shape, 13)
    ext = R.clahe_extend(img, *tiles)
    assert ext.shape[0] % tiles[1] == 0 and ext.shape[1] % tiles[0] == 0 and (ext[:shape[0], :shape[1]] == img).all()
    assert ext.shape[0] - shape[0] in (0, tiles[1] - shape[0] % tiles[1]) and ext.shape[1] - shape[1] in (0, tiles[0] - shape[1] % tiles[0])
    want = sv_oracle.clahe(np.ascontiguousarray(ext), 2.0, tiles)[:shape[0], :shape[1]]
    assert (R.clahe(img, 2.0, tiles) == want).all()


def _otsu_exhaustive(img):
    """argmax of the between-class variance in exact rational arithmetic -> (threshold, is the maximum unique)."""
    h = np.bincount(img.ravel(), minlength=256).tolist()
    N, S = sum(h), sum(i * v for i, v in enumerate(h))
    best, arg, ties = Fraction(0), 0, 0
    n0 = s0 = 0
    for t in range(256):
        n0 += h[t]
        s0 += t * h[t]
        if n0 == 0 or n0 == N:
            continue
        sigma = Fraction((s0 * N - S * n0) ** 2, n0 * (N - n0))
        if sigma > best:
            best, arg, ties = sigma, t, 1
        elif sigma == best:
            ties += 1
    return arg, ties == 1


@pytest.mark.parametrize("seed", range(8))
def test_otsu_equals_oracle_and_exhaustive_search(seed):
    rs = np.random.RandomState(seed)
    img = np.clip(np.where(rs.rand(40, 50) < 0.3, rs.normal(60 + 5 * seed, 15, (40, 50)), rs.normal(180, 25, (40, 50))), 0, 255).astype(np.uint8)
    t = R.otsu_threshold(img)
    assert t == sv_oracle.cell_ink_ratio(img)[1]
    want, unique = _otsu_exhaustive(img)
    if unique:
        assert t == want
    assert (R.threshold_otsu(img) == np.where(img > t, 0, 255)).all()
    hist = np.bincount(img.ravel(), minlength=256)
    assert _module().otsu_from_histogram(hist) == t


def test_otsu_constant_image():
    img = np.full((5, 5), 9, np.uint8)
    assert R.otsu_threshold(img) == sv_oracle.cell_ink_ratio(img)[1] == _module().otsu_from_histogram(np.bincount(img.ravel(), minlength=256)) == 0


def test_sauvola_close_to_float64():
    img = _img((60, 80), 3)
    f = img.astype(np.float64)
    mean = ndi.uniform_filter(f, 25, mode="mirror")
    std = np.sqrt(np.maximum(ndi.uniform_filter(f * f, 25, mode="mirror") - mean * mean, 0))
    t = mean * (1 + 0.2 * (std / 128 - 1))
    clear = np.abs(f - t) > 1e-3
    assert clear.mean() > 0.99
    assert (R.threshold_sauvola(img, 25, 0.2)[clear] == np.where(f < t, 255, 0)[clear]).all()


# ---- the drop-in's host side ------------------------------------------------------------------------------------------------------
def test_module_kernel_sizes_match():
    m = _module()
    for shape in [(1080, 1920), (2736, 3648), (912, 1216), (100, 80), (7, 1), (1, 1), (511, 1020)]:
        assert m.illumination_kernel_size(shape) == R.illumination_kernel_size(shape)
        assert m.shadow_kernel_size(shape) == R.shadow_kernel_size(shape)
        assert m.illumination_kernel_size(shape) % 2 == 1 and m.shadow_kernel_size(shape) % 2 == 1


def test_module_flags_from_counts():
    m = _module()
    assert m.glare_flag(101, 10000) is True and m.glare_flag(100, 10000) is False            # > 0.01, strictly
    assert m.shadow_flag(500, 10000) is False and m.shadow_flag(501, 10000) is True          # > 0.05, strictly
    assert m.shadow_flag(4999, 10000) is True and m.shadow_flag(5000, 10000) is False        # < 0.5, strictly
    for shape, seed in [((40, 50), 0), ((64, 64), 1)]:
        g = _img(shape, seed)
        assert m.glare_flag(np.count_nonzero(g > 250), g.size) == R.detect_glare(g)[0]


def test_module_strategy_scoring_and_choice():
    m = _module()
    n = 100000
    assert m.score_binary_count(1999, n) == 0 and m.score_binary_count(30001, n) == 0
    assert m.score_binary_count(2000, n) == 0                     # (255 * 0.02) / 255 rounds to just below 0.02 in float64: np.mean(b) / 255 does the same
    assert m.score_binary_count(2100, n) == pytest.approx(0.21) and m.score_binary_count(10000, n) == pytest.approx(1.0)
    assert m.score_binary_count(30000, n) == pytest.approx(-1.0)                               # the reference's score goes negative above 20 %
    assert m.METHODS == ("adaptive", "otsu", "sauvola")
    assert m.choose_strategy([10000, 10000, 10000], n) == 0                                    # first maximum
    assert m.choose_strategy([0, 0, 0], n) == 0
    assert m.choose_strategy([500, 9000, 12000], n) == 1
    assert m.choose_strategy([500, 15000, 11000], n) == 2
    assert m.choose_strategy([25000, 100, 50000], n) == 1                                      # 0 beats a negative score
    rs = np.random.RandomState(0)
    for _ in range(50):
        counts = rs.randint(0, n, 3)
        imgs = []
        for c in counts:
            b = np.zeros(n, np.uint8)
            b[:c] = 255
            imgs.append(b)
        scores = [R.score_binary(b) for b in imgs]
        assert [m.score_binary_count(c, n) for c in counts] == scores
        assert m.choose_strategy(counts, n) == max(range(3), key=lambda i: scores[i])


def test_dropin_preprocess_v2_names_resolve():
    """run_v2 does sys.path.insert(cv/) and `from preprocess_v2 import ...` (pipeline/run_v2.py:37)."""
    code = ("import sys; sys.path.insert(0, %r);"
            "from preprocess_v2 import %s;"
            "import preprocess_v2, dataclasses;"
            "assert [f.name for f in dataclasses.fields(PreprocessResult)] == ['binary', 'gray', 'enhanced', 'illumination_normalized', 'has_glare', 'has_shadow', 'method_used'];"
            "r = PreprocessResult(None, None, None); assert (r.illumination_normalized, r.has_glare, r.has_shadow, r.method_used) == (None, False, False, 'adaptive');"
            "print('ok')") % (CV_DIR, ", ".join(NAMES))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_dropin_signatures_match_the_reference_defaults():
    import inspect
    m = _module()
    want = {"grayscale": "(image)", "normalize_illumination": "(gray)", "detect_glare": "(gray, threshold: int = 250)", "detect_shadow": "(gray)",
            "remove_shadow": "(gray)", "apply_clahe": "(gray, clip_limit: float = 2.0, tile_size: int = 8)",
            "threshold_adaptive": "(gray, block_size: int = 11, c: int = 2)", "threshold_otsu": "(gray)",
            "threshold_sauvola": "(gray, window_size: int = 25, k: float = 0.2)",
            "morphological_cleanup": "(binary, close_size: int = 3, open_size: int = 2)",
            "preprocess_for_grid_detection": "(image, use_illumination_norm: bool = True, use_shadow_removal: bool = True)",
            "preprocess_multi_strategy": "(image)", "preprocess_cell": "(cell, clip_limit: float = 2.0, tile_size: int = 4)"}
    for name, sig in want.items():
        assert str(inspect.signature(getattr(m, name))) == sig, name
