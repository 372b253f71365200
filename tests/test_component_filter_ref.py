"""CPU: the component filter's definition (tests/component_filter_ref.py, a restatement in scipy) is exact for the product's host corner
search -- find_grid_corners(filter(b, r), r') == find_grid_corners(b, r') for r' >= r, with the byte and the bit scanner --, its threshold
cases, and the two C-ABI symbols' argument checks, which need no GPU.  tests/test_gpu_component_filter.py compares the kernels with the
same restatement bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import component_filter_ref as R
import despeckle_ref as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def host():
    import sudoku_vision_amd as sva
    sva._native.lib()
    return sva.host


def _search(host, img, r):
    """Corners by the byte scanner, and by the bit scanner too where the width allows; the two must agree."""
    img = np.asarray(img) != 0
    H, W = img.shape
    got = host.find_grid_corners(img.astype(np.uint8) * 255, r)
    got = None if got is None else got.tolist()
    if W % 32 == 0:
        c, f = host.find_grid_corners_bits_batch(R.pack_bits(img)[None], H, W, r, threads=1)
        assert (c[0].tolist() if f[0] else None) == got
    return got


def _inputs():
    out = [("grid+noise", D.rectangle_outline(192, 288, 20, 150, 30, 230) | R.noise(0.05, 1, (192, 288)), 0.1),
           ("percolation 0.38", R.noise(0.38, 2, (192, 288)), 0.1), ("percolation 0.5", R.noise(0.5, 3, (192, 288)), 0.1),
           ("percolation 0.6", R.noise(0.6, 4, (192, 288)), 0.05), ("rings", R.rings(192, 288), 0.1), ("lattice", R.lattice(192, 288), 0.1),
           ("comb", R.comb(192, 288), 0.1), ("spiral", R.frame_spiral(192, 288), 0.1), ("isolated", R.isolated(192, 288), 0.1),
           ("odd width", D.rectangle_outline(130, 250, 10, 100, 12, 200) | R.noise(0.3, 5, (130, 250)), 0.1),
           ("topology", D.case_topology()[0][0], 0.1), ("quad", _quad(192, 288), 0.1)]
    frames, _, _ = R.threshold_frames(192, 288, 0.25)
    return out + [(f"threshold {i}", f, 0.25) for i, f in enumerate(frames)]


def _quad(H, W):
    """A filled, slightly rotated quadrilateral (found by the search) among specks."""
    y, x = np.mgrid[:H, :W]
    q = (y - 0.1 * x > 10) & (y - 0.1 * x < 140) & (x + 0.1 * y > 40) & (x + 0.1 * y < 240)
    return q | D.specks(H, W, 9)


@pytest.mark.parametrize("name,img,r", _inputs(), ids=[c[0] for c in _inputs()])
def test_filter_is_exact_for_the_host_search(host, name, img, r):
    filt = R.component_filter(img, r)
    assert not (filt & ~img).any()
    for r2 in (r, min(2.5 * r, 0.9)):
        assert _search(host, filt, r2) == _search(host, img, r2), (name, r2)
    if name in ("grid+noise", "quad", "topology", "threshold 0"):
        assert _search(host, img, r) is not None                          # the comparison is not one of None with None throughout


@pytest.mark.parametrize("i", range(1, 6))
def test_filter_is_exact_on_the_reference_photos(host, i):
    """The K1 binaries of the five photos, obtained as tests/test_host_contours.py does (the C oracle's K1)."""
    o = pytest.importorskip("sv_oracle")
    Image = pytest.importorskip("PIL.Image")
    img = np.asarray(Image.open(os.path.join(GOLDEN, f"sample_{i}.jpg")).convert("RGB"))[..., ::-1].copy()
    b = o.preprocess_for_grid_detection(img)
    filt = R.component_filter(b, 0.1)
    assert R.count_components(filt) <= 3 < R.count_components(b)
    for r2 in (0.1, 0.2):
        want = host.find_grid_corners(b, r2)
        got = host.find_grid_corners(filt, r2)
        assert (want is None) == (got is None) and (want is None or (want == got).all())


def test_threshold_cases():
    """64x64 at ratio 0.25: the floor is exactly 1024.0.  Box differences 32x32 (1024) stay, 31x33 (1023) go, and a line one pixel high
    or wide has a zero product and goes for any positive floor."""
    frames, kept, under = R.threshold_frames(64, 64, 0.25)
    assert 0.25 * (64.0 * 64.0) == 1024.0 and kept == (32, 32) and under == (31, 33)
    assert np.array_equal(R.component_filter(frames[0], 0.25), frames[0])
    assert not R.component_filter(frames[1], 0.25).any()
    assert not R.component_filter(frames[2], 0.25).any() and not R.component_filter(frames[2], 1e-9).any()
    assert np.array_equal(R.component_filter(frames[1], 1023.0 / 4096.0), frames[1])
    both = frames[0] | np.roll(frames[2], -2, axis=0)                       # the line two rows up, clear of nothing else: only it goes
    both[:, 0] = False
    assert np.array_equal(R.component_filter(both, 0.25), frames[0])


def test_ratio_zero_is_the_identity():
    for img in (R.noise(0.3, 7, (67, 61)), R.isolated(40, 64), np.ones((5, 1), bool)):
        assert np.array_equal(R.component_filter(img, 0.0), img)
    u8 = (R.noise(0.3, 8, (20, 33)) * np.arange(1, 34, dtype=np.uint8)).astype(np.uint8)     # kept pixels keep their values
    assert np.array_equal(R.component_filter(u8, 0.0), u8)


def test_symbols_check_their_arguments_without_a_gpu():
    """sv_component_filter_bits / _u8 are exported, and refuse bad arguments before anything touches the context or the device."""
    import sudoku_vision_amd as sva
    lib = sva._native.lib()
    ctx = C.c_void_p(0x1000)                                                  # never dereferenced: every call below fails its checks first
    buf = np.zeros(64, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    BAD, UNSUPPORTED = -1, -4
    assert lib.sv_component_filter_bits(None, p, 1, 4, 32, 0.1, None) == BAD
    assert lib.sv_component_filter_bits(ctx, None, 1, 4, 32, 0.1, None) == BAD
    assert lib.sv_component_filter_bits(ctx, p, -1, 4, 32, 0.1, None) == BAD
    assert lib.sv_component_filter_bits(ctx, p, 1, 0, 32, 0.1, None) == BAD
    assert lib.sv_component_filter_bits(ctx, p, 1, 4, 32, -0.1, None) == BAD
    assert lib.sv_component_filter_bits(ctx, p, 1, 4, 32, float("nan"), None) == BAD
    assert lib.sv_component_filter_bits(ctx, p, 1, 4, 40, 0.1, None) == UNSUPPORTED
    assert b"multiple of 32" in lib.sv_last_error()
    assert lib.sv_component_filter_bits(ctx, p, 0, 4, 32, 0.1, None) == 0        # n == 0: a no-op
    assert lib.sv_component_filter_u8(None, p, 1, 4, 32, 0.1, p, None, None) == BAD
    assert lib.sv_component_filter_u8(ctx, p, 1, 4, 32, 0.1, None, None, None) == BAD
    assert lib.sv_component_filter_u8(ctx, None, 1, 4, 32, 0.1, p, None, None) == BAD
    assert lib.sv_component_filter_u8(ctx, p, 1, 4, -3, 0.1, p, None, None) == BAD
    assert lib.sv_component_filter_u8(ctx, p, 1, 4, 32, float("nan"), p, None, None) == BAD
    assert lib.sv_component_filter_u8(ctx, p, 1, 4, 33, 0.1, p, p, None) == BAD    # packed needs W % 32 == 0
    assert lib.sv_component_filter_u8(ctx, p, 0, 4, 33, 0.1, p, None, None) == 0
    assert lib.sv_version() == 2
