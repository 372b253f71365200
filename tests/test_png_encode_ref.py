"""CPU: tests/png_encode_ref.py, the restatement the PNG encoder's GPU tests use as their oracle, against Pillow: a file built from the
restatement's filtered bytes with Python's zlib decodes to exactly the input, for each fixed filter and for adaptive; the adaptive choice follows
the stated rule, ties included."""
import numpy as np
import pytest

import png_encode_ref as R

SHAPES = [(1, 1), (5, 1), (5, 7), (37, 53), (48, 80)]                  # (H, W)


@pytest.mark.parametrize("mode", R.FILTERS)
def test_filtered_bytes_decode_to_the_input(mode):
    for H, W in SHAPES:
        for gray in (False, True):
            for kind in ("noise", "synthetic", "flat", "zeros"):
                img = R.content(kind, H, W, gray)
                f = R.filtered(img, mode)
                assert len(f) == H * (1 + W * (1 if gray else 3))
                data = R.make_file(img, R.zlib_rle(f))
                assert R.check_file(data, img) == f
                got, pmode, size = R.pillow_decode(data)
                assert pmode == ("L" if gray else "RGB") and size == (W, H)
                assert (got == img).all(), (mode, H, W, gray, kind)


def test_fixed_filters_write_their_number():
    img = R.content("synthetic", 9, 11)
    for k, mode in enumerate(R.FILTERS[:5]):
        rows = np.frombuffer(R.filtered(img, mode), np.uint8).reshape(9, -1)
        assert (rows[:, 0] == k).all()
    assert (np.frombuffer(R.filtered(img, "none"), np.uint8).reshape(9, -1)[:, 1:] == img[:, :, ::-1].reshape(9, -1)).all()


def test_adaptive_rule_and_ties():
    # all zero: every filter gives sum 0 -> None (0), the lowest number
    assert (R.row_filters(np.zeros((4, 6), np.uint8), "adaptive") == 0).all()
    # a constant row of 100 over a zero row: None 6 * 100; Sub 100; Up 6 * 100; Average 100 + 5 * 50; Paeth 100 -> Sub (1) before Paeth (4)
    img = np.zeros((2, 6), np.uint8)
    img[1] = 100
    assert list(R.row_filters(img, "adaptive")) == [0, 1]
    # the second of two equal rows: Up is all zero, and so is nothing else
    img = np.stack([np.arange(10, 70, 10, dtype=np.uint8)] * 2)
    assert R.row_filters(img, "adaptive")[1] == 2
    # abs((int8) b): 255 counts as 1, 128 as 128
    img = np.array([[255, 255, 255, 255]], np.uint8)                    # None: 4; Sub: 1 + 0 -> Sub
    assert list(R.row_filters(img, "adaptive")) == [1]
    # every filter is chosen somewhere on the synthetic frame
    assert set(R.row_filters(R.content("synthetic", 48, 80), "adaptive")) >= {1, 2, 4}
