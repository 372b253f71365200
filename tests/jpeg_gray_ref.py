"""libjpeg's grayscale read of a JPEG file (out_color_space = JCS_GRAYSCALE: cv2.imread(path, cv2.IMREAD_GRAYSCALE) and
IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8, Pillow's Image.draft('L', ...)) restated in numpy: the Y component alone through the scaled inverse
DCTs tests/jpeg_reduced_ref.py restates, the range limit, the crop to ceil(H / d) x ceil(W / d), the EXIF orientation.  Cb and Cr are
never looked at, so the result is NOT the gray conversion of the colour decode (tests/test_jpeg_gray_ref.py records the difference).
Independent of csrc/k20_jpeg_gray.hip and of csrc/host_jpeg.cpp's luma mode: the coefficients come from the oracle's entropy decoder.

Also the Pillow leg, pil_gray(): draft('L', size) flips the same libjpeg switch.  Pillow picks its scale as min(W // w, H // h), so the size
to ask for is (W // d, H // d), never below 1x1, and the size it answers with is asserted to be the ceil size: an unreduced decode cannot
pass for a reduced one.  A file with a side shorter than d cannot be reduced by d through draft(); pil_can_reduce() says which can."""
import io

import numpy as np

import jpeg_reduced_ref as R

SCALES = R.SCALES


def luma_blocks(coef, width, height, hmax, vmax):
    """Y's blocks [bh, bw, 64] from the full decode's layout (component after component, padded block grid row-major)"""
    bw, bh = R.ceil_div(width, 8 * hmax) * hmax, R.ceil_div(height, 8 * vmax) * vmax
    return np.asarray(coef).ravel()[:64 * bw * bh].reshape(bh, bw, 64)


def scan_order(blocks, hmax, vmax):
    """[bh, bw, 64] raster -> [bh * bw, 64] in scan order: MCU after MCU, an MCU's hmax x vmax blocks row-major (the luma-only records)"""
    bh, bw, _ = blocks.shape
    return blocks.reshape(bh // vmax, vmax, bw // hmax, hmax, 64).transpose(0, 2, 1, 3, 4).reshape(-1, 64)


def orient_gray(img, orientation):
    return R.orient(img[..., None], orientation)[..., 0]


def decode_gray(coef, quant, width, height, hmax, vmax, orientation, d):
    """coefficients in the full decode's layout, quantiser steps [ncomp, 64] -> uint8 [ceil(H/d), ceil(W/d)] under the orientation"""
    assert d in SCALES
    S = 8 // d
    blocks = luma_blocks(coef, width, height, hmax, vmax).astype(np.int64)
    bh, bw, _ = blocks.shape
    deq = blocks.reshape(-1, 64) * np.asarray(quant, np.int64).reshape(-1, 64)[0]
    plane = R.idct_blocks(deq.reshape(-1, 8, 8), S).reshape(bh, bw, S, S).transpose(0, 2, 1, 3).reshape(bh * S, bw * S)
    ow, oh = R.scaled_size(width, height, d)
    return orient_gray(plane[:oh, :ow], orientation)


def decode_file(data, d):
    """a JPEG file through the oracle's entropy decoder and the rule above"""
    import sv_oracle as o
    info = o.jpeg_info(data)
    coef, quant = o.jpeg_coefficients(data)
    return decode_gray(coef, quant, info.width, info.height, info.h_samp, info.v_samp, info.orientation, d)


def pil_can_reduce(width, height, d):
    return d == 1 or (width >= d and height >= d)


def pil_gray(data, d):
    """Pillow's luma-only decode at scale 1 / d (orientation NOT applied: Pillow leaves it to the caller)"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    w, h = im.size
    assert pil_can_reduce(w, h, d), "draft cannot reduce a side shorter than d by d"
    im.draft("L", (max(1, w // d), max(1, h // d)))
    assert im.mode == "L" and im.size == (R.ceil_div(w, d), R.ceil_div(h, d)), "Pillow did not decode luma-only at 1 / d"
    return np.asarray(im)


def pil_gray_oriented(data, d):
    import sv_oracle as o
    return orient_gray(pil_gray(data, d), o.jpeg_info(data).orientation)
