"""GPU (-m gpu): K5 (csrc/k5_jpeg.hip: k_jpeg_idct<SPARSE>, k_jpeg_colour) on the crafted files of tests/test_jpeg_crafted.py, which
checks on the CPU that Pillow opens them, that the oracle agrees with it and that the host decoder returns the written coefficients.
Here every file goes through Context.imdecode with both transports and must equal Pillow's libjpeg-turbo decode in every pixel."""
import numpy as np
import pytest
import torch

import sv_oracle as o
import test_jpeg_crafted as T
from test_jpeg import encode, pil_bgr, synth_image

pytestmark = pytest.mark.gpu


def gpu_both(ctx, data):
    """the decode through the compact and through the dense transport"""
    return [(dense, ctx.imdecode(data, dense=dense).cpu().numpy()) for dense in (False, True)]


def assert_equals_pillow(ctx, data):
    want = pil_bgr(data)
    for dense, got in gpu_both(ctx, data):
        assert got.shape == want.shape and (got == want).all(), f"dense={dense}"


@pytest.mark.parametrize("luma", T.A_LUMA)
def test_a_colour_conversion_exhaustive(ctx, luma):
    """every (Cb, Cr) pair at Y = 0, Y = 255 or a Y that varies: both clamp arms of every channel, every rounding of the >> 16"""
    assert_equals_pillow(ctx, T.file_a(luma).data)


@pytest.mark.parametrize("sampling", ["4:2:0", "4:2:2"])
@pytest.mark.parametrize("pattern", T.B_PATTERNS)
def test_b_chroma_upsampling_hard_chroma(ctx, sampling, pattern):
    """chroma alternating 0/255 per sample: where a wrong rounding constant of chroma_sample changes the most pixels"""
    for w, h in T.B_SIZES:
        assert_equals_pillow(ctx, T.file_b(w, h, sampling, pattern).data)


@pytest.mark.parametrize("sampling", ["gray", "4:2:0"])
def test_c_sparse_rank_selection(ctx, sampling):
    """blocks with all 64 positions set, none, only zigzag 63, 62 and 63, the lower and the upper half; with restart intervals too"""
    for interval in (0, 2):
        assert_equals_pillow(ctx, T.file_c(sampling, interval).data)


def test_d_range_limit(ctx):
    """One flat block per sample value 128 + k (tests/test_jpeg_crafted.py::test_d_range_limit).  Where the oracle equals Pillow --
    measured: every k of the file from -400 to 496, sample values clamped to 0 and to 255 included -- Pillow is the judge; at k = 512 and
    520, where libjpeg-turbo's SIMD code saturates to 255 and libjpeg's table (the oracle, the kernel) wraps to 0, the oracle alone."""
    f = T.file_d()
    agree = np.repeat(T.d_agreement(), 8)                                    # per pixel column
    ks = np.array(T.d_offsets())
    assert T.d_agreement()[ks <= 511].all()
    pil, ora = pil_bgr(f.data), o.imdecode(f.data)
    for dense, got in gpu_both(ctx, f.data):
        assert (got[:, agree] == pil[:, agree]).all(), f"dense={dense}"
        assert (got == ora).all(), f"dense={dense}"


@pytest.mark.parametrize("sampling,w,h", T.E_CASES)
def test_e_block_counts_and_component_boundaries(ctx, sampling, w, h):
    """31, 32 and 33 blocks; the Y/Cb and Cb/Cr boundaries inside a 32-block workgroup; every block a different flat value"""
    assert_equals_pillow(ctx, T.file_e(sampling, w, h).data)


@pytest.mark.parametrize("h,w", T.F_SHAPES)
def test_f_orientations_wide(ctx, h, w):
    """More than one 256-thread workgroup per output row under every orientation.  (300, 9) is the file that tells orientation 6 from 8
    beyond ox = 255: its output rows are 300 wide, W != H, and the two formulas read the source column and row the other way round."""
    for orient in range(1, 9):
        for sub in (0, 1, 2):
            data = T.file_f(h, w, orient, sub)
            want = pil_bgr(data)
            assert want.shape == ((w, h, 3) if orient >= 5 else (h, w, 3))
            assert (o.imdecode(data) == want).all(), (orient, sub)
            for dense, got in gpu_both(ctx, data):
                assert got.shape == want.shape and (got == want).all(), (orient, sub, dense)


@pytest.mark.parametrize("sampling,w,h,orient", T.F_CRAFTED)
def test_f_orientations_crafted(ctx, sampling, w, h, orient):
    assert_equals_pillow(ctx, T.file_e(sampling, w, h, orient).data)


@pytest.mark.parametrize("orient", [1, 6])
def test_g_out_with_pitch(ctx, orient):
    """imdecode(out=view) into a strided [H, W, 3] view -- padded rows, odd byte offset -- of a larger buffer: the view holds Pillow's
    pixels and not one byte around it changes.  (imdecode accepts such a view: out.stride(0) is the kernel's row pitch.)"""
    from PIL import Image
    exif = Image.Exif()
    exif[0x0112] = orient
    data = encode(synth_image(61, 83, 61 * 131 + 83), quality=75, subsampling=2, exif=exif)
    want = pil_bgr(data)
    H, W = want.shape[:2]
    assert (H, W) == ((83, 61) if orient == 6 else (61, 83))
    pitch, offset = 3 * W + 37, 1001
    for dense in (False, True):
        buf = torch.full((offset + H * pitch + 333,), 0xA5, dtype=torch.uint8, device=ctx.device)
        view = torch.as_strided(buf, (H, W, 3), (pitch, 3, 1), offset)
        ret = ctx.imdecode(data, out=view, dense=dense)
        assert ret.data_ptr() == view.data_ptr()
        host = buf.cpu().numpy()
        inside = np.zeros(host.shape, bool)
        rows = offset + pitch * np.arange(H)
        inside[(rows[:, None] + np.arange(3 * W)).ravel()] = True
        assert (host[inside].reshape(H, W, 3) == want).all(), f"dense={dense}"
        assert (host[~inside] == 0xA5).all(), f"dense={dense}"
