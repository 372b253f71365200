"""CPU: tests/threshold_ref.py (an independent numpy restatement of K1) against the C oracle on every threshold_ref.CASES entry and
on random shapes, its exact f32 fma against libm's fmaf, closed forms (the fused kernels' f32 gray on all 2^24 colours, flat
images, period-2 stripes), and the mutations: every rule the restatement states is exercised by CASES, and the tie-dense inputs
hold enough order-sensitive pixels that a bit-exact comparison sees a wrong operation order -- which the older noise inputs do
not."""
import ctypes
import ctypes.util
import functools

import numpy as np
import pytest

import sv_oracle as o
import threshold_ref as T

GRAY_CASES = [c for c in T.CASES if c.kind == "gray"]
FRAME_CASES = [c for c in T.CASES if c.kind == "frame"]


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert not bad.size, f"{what}: {len(bad)} mismatches, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"


def test_taps_equal_oracle_and_unfused_sigma():
    for n in (1,) + T.BLOCKS:
        k = T.gaussian_kernel_f32(n)
        assert k.tobytes() == o.gaussian_kernel_f32(n).tobytes(), n
        # OpenCV's fused sigma (n*0.15 + 0.35) and the textbook 0.3*((n-1)/2 - 1) + 0.8 give the same float taps here
        assert k.tobytes() == T.gaussian_kernel_f32(n, fused_sigma=False).tobytes(), n


@pytest.mark.parametrize("case", GRAY_CASES, ids=lambda c: c.name)
def test_standalone_stages_equal_oracle(case):
    imgs = case.data()
    for k in (1, 3, 5, 7):
        _same(T.blur(imgs, k), np.stack([o.gaussian_blur(x, k) for x in imgs]), f"{case.name} blur {k}")
    for block in T.BLOCKS:
        mean = T.adaptive_mean(imgs, block)
        _same(mean, np.stack([o.adaptive_mean(x, block) for x in imgs]), f"{case.name} mean {block}")
        for c in T.C_VALUES:
            for inv in (True, False):
                _same(T.threshold_from_mean(imgs, mean, c, inv), np.stack([o.adaptive_threshold(x, block, c, inv) for x in imgs]),
                      f"{case.name} threshold {block} C={c} inv={inv}")


@pytest.mark.parametrize("case", FRAME_CASES, ids=lambda c: c.name)
def test_fused_path_equals_oracle(case):
    frames = case.data()
    _same(T.gray(frames), np.stack([o.gray(f) for f in frames]), f"{case.name} gray")
    _same(T.preprocess(frames), np.stack([o.preprocess_for_grid_detection(f) for f in frames]), f"{case.name} preprocess")


def test_random_shapes_equal_oracle():
    rs = np.random.RandomState(40)
    shapes = [(1, 1), (1, 2), (2, 1), (1, 37), (37, 1), (2, 2), (3, 5), (4, 4)] + [tuple(rs.randint(1, 48, 2)) for _ in range(14)]
    for H, W in shapes:
        bgr = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        g = o.gray(bgr)
        _same(T.gray(bgr), g, f"gray {H}x{W}")
        for k in (3, 5, 7):
            _same(T.blur(g, k), o.gaussian_blur(g, k), f"blur {k} {H}x{W}")
        for block in (3, 5, 7, 11, 21, 31):
            _same(T.adaptive_mean(g, block), o.adaptive_mean(g, block), f"mean {block} {H}x{W}")
        _same(T.preprocess(bgr), o.preprocess_for_grid_detection(bgr), f"preprocess {H}x{W}")


# ---- the exact fma ---------------------------------------------------------------------------------------------------------------
def _libm_fmaf():
    f = ctypes.CDLL(ctypes.util.find_library("m")).fmaf
    f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    return f


def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def test_fma_equals_libm():
    fmaf = _libm_fmaf()
    rs = np.random.RandomState(41)
    n = 1 << 20
    sign = lambda: np.where(rs.randint(0, 2, n) == 1, np.float32(-1), np.float32(1))
    a = (rs.uniform(0, 512, n).astype(np.float32) * sign()).astype(np.float32)
    b = _f32(rs.randint(0x3a000000, 0x3f800000, n, dtype=np.int64))          # taps-like magnitudes 5e-4 .. 1
    c = (rs.uniform(0, 300, n).astype(np.float32) * sign()).astype(np.float32)
    wide = rs.randint(0, 2, n) == 1                                               # half of them: exponents far apart
    c = np.where(wide, _f32(rs.randint(0x20000000, 0x5f000000, n, dtype=np.int64)) * sign(), c).astype(np.float32)
    got = T.fma_f32(a, b, c)
    want = np.array([fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], np.float32)
    _same(got.view(np.uint32), want.view(np.uint32), "fma_f32 vs fmaf")


def test_fma_midpoint_cases():
    """a*b = half an ulp of c, less (or more) than 2^-40 of it: a float64 fma rounded to f32 lands exactly on the tie and rounds to
    even; the true result does not."""
    fmaf = _libm_fmaf()
    rs = np.random.RandomState(42)
    cs = _f32((rs.randint(0x3f800000, 0x4e800000, 2000, dtype=np.int64) | 1))    # odd mantissas in [1, 2^30)
    ulp = (np.nextafter(cs, np.float32(np.inf)) - cs).astype(np.float64)
    A, B, C = [], [], []
    for c, u in zip(cs, ulp):
        for a, bf in ((1 + 2.0 ** -23, 1 - 2.0 ** -23), (1 - 2.0 ** -24, 1 + 2.0 ** -23), (1.0, 1.0), (1 + 2.0 ** -22, 1 - 2.0 ** -22)):
            for s in (1, -1):
                A.append(a)
                B.append(s * u / 2 * bf)
                C.append(c)
    A, B, C = (np.array(v, np.float32) for v in (A, B, C))
    assert (B.astype(np.float64) * A.astype(np.float64) != 0).all()
    want = np.array([fmaf(x, y, z) for x, y, z in zip(A.tolist(), B.tolist(), C.tolist())], np.float32)
    _same(T.fma_f32(A, B, C).view(np.uint32), want.view(np.uint32), "fma_f32 midpoints")
    naive = (A.astype(np.float64) * B.astype(np.float64) + C.astype(np.float64)).astype(np.float32)
    assert (naive != want).sum() > 1000          # the cases are real: double rounding gets these wrong


# ---- closed forms -------------------------------------------------------------------------------------------------------------
def test_f32_gray_formula_on_all_colours():
    """The fused kernels' gray, floor(fma(b, 3735/2^15, fma(g, 19235/2^15, fma(r, 9798/2^15, 0.5)))), equals the integer
    formula on all 2^24 BGR triples (every intermediate is exact in f32)."""
    g, r = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    g, r = g.ravel(), r.ravel()
    for b in range(0, 256, 16):
        bb = np.repeat(np.arange(b, b + 16), g.size)
        gg, rr = np.tile(g, 16), np.tile(r, 16)
        want = ((3735 * bb + 19235 * gg + 9798 * rr + 16384) >> 15).astype(np.uint8)
        _same(T.gray_f32_formula(bb, gg, rr), want, f"gray b={b}..{b + 15}")
        _same(T.gray(np.stack([bb, gg, rr], -1)), want, "gray integer")


def test_flat_images_mean_is_the_value():
    flat = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 7 * 9, 1).reshape(256, 7, 9)
    for block in T.BLOCKS:
        _same(T.adaptive_mean(flat, block), flat, f"flat mean {block}")


def test_stripes_round_half_to_even():
    """Period-2 stripes a, b with a + b odd: inside, the dyadic blocks 3/5/7 give the exact mean (a + b)/2, rounded to even."""
    for a, b in ((100, 103), (7, 10), (0, 255), (254, 1)):
        for axis in (0, 1):
            img = T._stripes(21, 21, a, b, axis)
            want = np.rint((a + b) / 2)
            assert want % 2 == 0
            for block in (3, 5, 7):
                r = block // 2
                for m in (T.adaptive_mean(img, block), o.adaptive_mean(img, block)):
                    assert (m[r:-r, r:-r] == want).all(), (a, b, axis, block)
                assert (T.adaptive_mean(img, block, "round_half_away")[r:-r, r:-r] == (a + b) // 2 + 1).all()


# ---- mutations and fragility ------------------------------------------------------------------------------------------------------
def _outputs(mutation):
    """Every output CASES produces under `mutation`: blur of the gray cases, threshold of each at the blocks and C values that
    matter, gray and preprocess of the frame cases."""
    out = []
    for case in GRAY_CASES:
        imgs = case.data()
        for k in (3, 5, 7):
            out.append(T.blur(imgs, k, mutation))
        for block in (case.params.get("block", 11), 3, 11, 31):
            for c, inv in ((2, True), (2, False), (2.5, True), (2.5, False), (-1.5, True)):
                out.append(T.adaptive_threshold(imgs, block, c, inv, mutation))
    for case in FRAME_CASES:
        frames = case.data()
        out += [T.gray(frames, mutation), T.preprocess(frames, mutation)]
    return out


@functools.lru_cache(maxsize=None)
def _base_outputs():
    return _outputs(None)


@pytest.mark.parametrize("mutation", sorted(T.MUTATIONS))
def test_mutation_is_detected(mutation):
    assert any((a != b).any() for a, b in zip(_base_outputs(), _outputs(mutation))), f"CASES does not notice {mutation}"


# pixels each ORDER_MUTATION flips (measured: fused_tie 36 / 40 / 52, tie_b11 42 / 20 / 48, tie cells 5 / 3 / 11 of
# no_fma / row_centre_first / col_left_to_right); the floors keep the bit-exact GPU comparisons able to see an order error
FLOORS = {
    "fused_tie": {"no_fma": 28, "row_centre_first": 30, "col_left_to_right": 40},
    "tie_b11": {"no_fma": 32, "row_centre_first": 15, "col_left_to_right": 36},
    "cells": {"no_fma": 4, "row_centre_first": 2, "col_left_to_right": 8},
}


def _flips(family, mutation):
    if family == "fused_tie":
        f = T.BY_NAME["fused_tie"].data()
        return int((T.preprocess(f) != T.preprocess(f, mutation)).sum())
    if family == "tie_b11":
        g = T.BY_NAME["tie_b11"].data()
        return int((T.adaptive_threshold(g, 11, 2, True) != T.adaptive_threshold(g, 11, 2, True, mutation)).sum())
    _, cl = T.order_sensitive_cells(o.clahe, T.tie_cells())
    return int((T.adaptive_threshold(cl, 11, 2, False) != T.adaptive_threshold(cl, 11, 2, False, mutation)).sum())


@pytest.mark.parametrize("family", sorted(FLOORS))
def test_order_mutations_flip_the_tie_cases(family):
    counts = {m: _flips(family, m) for m in T.ORDER_MUTATIONS}
    print(family, counts)
    for m, floor in FLOORS[family].items():
        assert counts[m] >= floor, (family, m, counts[m], floor)


def test_noise_inputs_do_not_see_the_order():
    """The gap the tie cases close: on the noise frames test_preprocess_random_noise_bit_exact uses, a kernel without fused
    multiply-adds (or with another summation order) gives the same binary almost everywhere, so bit-exactness there proves
    little about the order."""
    f = T.BY_NAME["fused_noise"].data()
    base = T.preprocess(f)
    for m in T.ORDER_MUTATIONS:
        assert int((T.preprocess(f, m) != base).sum()) <= 2, m


def test_committed_tie_data():
    """tests/golden/k1_tie_patches.npz: every gray patch and cell is a tie to 4e-6, and the search reproduces the first ones."""
    g = T.tie_gray_patches()
    m, s = T._blur_window_mean(g)
    assert g.shape == (T.GRAY_PATCH_COUNT, 15, 15) and (np.abs(s + 1.5 - m) < 4e-6).all()
    assert (T.make_tie_gray_patches(2) == g[:2]).all()
    cells = T.tie_cells()
    cl = np.stack([o.clahe(c) for c in cells]).astype(np.float64)
    res = cl[:, 14, 14] + 1.5 - (cl[:, 9:20, 9:20] * T._weights(11)).sum(axis=(1, 2))
    assert cells.shape == (T.CELL_COUNT, 28, 28) and (np.abs(res) < 4e-6).all()
    assert (T.make_tie_cells(o.clahe, 2) == cells[:2]).all()


def test_linear_tie_patches_are_ties():
    for block in (3, 5, 7):
        p = T.tie_patches(block, 8, 1).astype(np.float64)
        r = block // 2
        assert ((p * T._weights(block)).sum(axis=(1, 2)) == p[:, r, r] + 1.5).all(), block
    for block in (11, 15, 31):
        p = T.tie_patches(block, 4, 1).astype(np.float64)
        r = block // 2
        assert (np.abs((p * T._weights(block)).sum(axis=(1, 2)) - p[:, r, r] - 1.5) < 1e-6).all(), block


def test_ambiguous_stripes():
    """One column in seven of the stripes pattern has a mean within 1e-3 of src + 1.5 (what the matrix-pipe test needs)."""
    f = T.stripes_frame(40, 140)
    b = T.blur(T.gray(f), 5)
    m = T.mean_f32(b, 11).astype(np.float64)
    close = np.abs(m - b - 1.5)[20, 20:120] < 1e-3
    assert close.mean() > 1 / 8
