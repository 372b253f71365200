"""libjpeg's reduced-size decode (scale_denom 2, 4, 8: cv2.IMREAD_REDUCED_COLOR_*, Pillow's Image.draft) restated in numpy, integer
arithmetic throughout: coefficients + quantiser steps + geometry -> BGR image.  Independent of csrc/k5_jpeg.hip and csrc/sv_api.cpp;
tests/test_jpeg_reduced_ref.py holds it against Pillow bit for bit, tests/test_gpu_jpeg_reduced.py holds the kernels against Pillow too.

The rules (jdmaster.c, jidctred.c, jidctint.c, jdsample.c, jdcolor.c):
  output size      ceil(W / d) x ceil(H / d), then the EXIF orientation
  block size       luma S = 8 / d; every other component starts at S and doubles while it is below 8 and the doubled block still
                   divides the MCU in both directions -- 4:2:0 chroma is decoded at 2S (no up-sampling left), 4:2:2 chroma stays at S
  plane size       ceil(W * h_c * S_c / (hmax * 8)) x ceil(H * v_c * S_c / (vmax * 8))
  inverse DCTs     8x8 jidctint.c; 4x4, 2x2, 1x1 jidctred.c (CONST_BITS 13, PASS1_BITS 2)
  up-sampling      what remains is h2v1 (4:2:2): the "fancy" triangle filter; plain replication when the plane is at most 2 wide, and
                   at d = 8 (jdsample.c switches the fancy filters off when blocks are 1x1: its context rows do not exist there)
  colour           jdcolor.c's 16-bit fixed point
"""
import numpy as np

SCALES = (1, 2, 4, 8)


def ceil_div(a, b):
    return -(-a // b)


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def range_limit(x):
    """libjpeg's post-IDCT table: index (x & 1023), centred on 128"""
    v = np.asarray(x) & 1023
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896))).astype(np.uint8)


def scaled_size(width, height, d):
    return ceil_div(width, d), ceil_div(height, d)


def block_sizes(d, ncomp, hmax, vmax):
    """samples per side each component's blocks are reconstructed at (jdmaster.c); chroma sampling factors are 1x1"""
    S = 8 // d
    out = [S]
    for _ in range(ncomp - 1):
        sc = S
        while sc < 8 and (hmax * S) % (1 * sc * 2) == 0 and (vmax * S) % (1 * sc * 2) == 0:
            sc *= 2
        out.append(sc)
    return out


def _idct8_1d(i, shift):
    """one 8-point pass of jidctint.c over the sequence i[0..7] of arrays"""
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) * 8192, (i[0] - i[4]) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1, z2, z3, z4 = i[7] + i[1], i[5] + i[3], i[7] + i[3], i[5] + i[1]
    z5 = (z3 + z4) * 9633
    z3, z4 = z5 - z3 * 16069, z5 - z4 * 3196
    z1, z2 = -z1 * 7373, -z2 * 20995
    o0, o1, o2, o3 = i[7] * 2446 + z1 + z3, i[5] * 16819 + z2 + z4, i[3] * 25172 + z2 + z3, i[1] * 12299 + z1 + z4
    return [descale(v, shift) for v in (t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3)]


def _idct4_1d(i, shift):
    """jidctred.c, 4x4: position 4 is not read"""
    t0 = i[0] * 16384
    t2 = i[2] * 15137 - i[6] * 6270
    t10, t12 = t0 + t2, t0 - t2
    z1, z2, z3, z4 = i[7], i[5], i[3], i[1]
    a = -z1 * 1730 + z2 * 11893 - z3 * 17799 + z4 * 8697
    b = -z1 * 4176 - z2 * 4926 + z3 * 7373 + z4 * 20995
    return [descale(v, shift) for v in (t10 + b, t12 + a, t12 - a, t10 - b)]


def _idct2_1d(i, shift):
    """jidctred.c, 2x2: positions 0, 1, 3, 5, 7"""
    t10 = i[0] * 32768
    t0 = -i[7] * 5906 + i[5] * 6967 - i[3] * 10426 + i[1] * 29692
    return [descale(t10 + t0, shift), descale(t10 - t0, shift)]


def idct_blocks(deq, S):
    """dequantised blocks [n, 8, 8] (row, column) -> samples uint8 [n, S, S]"""
    d = np.asarray(deq, np.int64)
    if S == 1:
        return range_limit(descale(d[:, 0, 0], 3))[:, None, None]
    f, s1, s2 = {8: (_idct8_1d, 11, 18), 4: (_idct4_1d, 12, 19), 2: (_idct2_1d, 13, 20)}[S]
    ws = np.stack(f([d[:, k, :] for k in range(8)], s1), 1)                      # columns: [n, S, 8]
    return range_limit(np.stack(f([ws[:, :, k] for k in range(8)], s2), 2))      # rows: [n, S, S]


def upsample_h2v1(plane, out_width, fancy=True):
    """jdsample.c: h2v1_fancy_upsample; h2v1_upsample (replication) when the plane is at most 2 samples wide or fancy is off"""
    p = plane.astype(np.int64)
    dw = p.shape[1]
    out = np.empty((p.shape[0], 2 * dw), np.int64)
    if dw <= 2 or not fancy:
        out[:, 0::2] = out[:, 1::2] = p
    else:
        left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
        out[:, 0::2] = (3 * p + left + 1) >> 2
        out[:, 1::2] = (3 * p + right + 2) >> 2
        out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out[:, :out_width]


def ycc_to_bgr(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def orient(img, orientation):
    """EXIF tag 0x0112 applied the way imread applies it"""
    if orientation in (2, 3):
        img = img[:, ::-1]
    if orientation in (3, 4):
        img = img[::-1]
    if orientation == 5:
        img = img.transpose(1, 0, 2)
    if orientation == 6:
        img = img[::-1].transpose(1, 0, 2)
    if orientation == 7:
        img = img[::-1, ::-1].transpose(1, 0, 2)
    if orientation == 8:
        img = img[:, ::-1].transpose(1, 0, 2)
    return np.ascontiguousarray(img)


def component_planes(coef, quant, width, height, ncomp, hmax, vmax, d):
    """-> the cropped component planes libjpeg hands its up-sampler at scale 1/d"""
    coef = np.asarray(coef, np.int64).ravel()
    quant = np.asarray(quant, np.int64).reshape(-1, 64)
    mcux, mcuy = ceil_div(width, 8 * hmax), ceil_div(height, 8 * vmax)
    planes, off = [], 0
    for c, sc in enumerate(block_sizes(d, ncomp, hmax, vmax)):
        h, v = (hmax, vmax) if c == 0 else (1, 1)
        bw, bh = mcux * h, mcuy * v
        deq = coef[off:off + 64 * bw * bh].reshape(-1, 64) * quant[c]
        off += 64 * bw * bh
        full = idct_blocks(deq.reshape(-1, 8, 8), sc).reshape(bh, bw, sc, sc).transpose(0, 2, 1, 3).reshape(bh * sc, bw * sc)
        planes.append(full[:ceil_div(height * v * sc, vmax * 8), :ceil_div(width * h * sc, hmax * 8)])
    assert off == coef.size
    return planes


def decode_reduced(coef, quant, width, height, ncomp, hmax, vmax, orientation, d):
    """coefficients in the product's layout (per component, padded block grid row-major, 64 natural-order values per block), quantiser
    steps [ncomp, 64] natural order -> BGR uint8 [ceil(H/d), ceil(W/d), 3] under the orientation"""
    assert d in SCALES and ncomp in (1, 3)
    ow, oh = scaled_size(width, height, d)
    planes = component_planes(coef, quant, width, height, ncomp, hmax, vmax, d)
    assert planes[0].shape == (oh, ow)
    if ncomp == 1:
        img = np.repeat(planes[0][..., None], 3, 2)
    else:
        chroma = []
        for p in planes[1:]:
            if p.shape != (oh, ow):                                               # at d > 1 only h2v1 can remain
                assert p.shape == (oh, ceil_div(ow, 2)) or d == 1
                p = upsample_h2v1(p, ow, fancy=d < 8) if p.shape[0] == oh else None
                assert p is not None, "h2v2 up-sampling: not a reduced decode"
            chroma.append(p)
        img = ycc_to_bgr(planes[0], *chroma)
    return orient(img, orientation)


def decode_file(data, d):
    """a JPEG file through the oracle's entropy decoder and the rules above"""
    import sv_oracle as o
    info = o.jpeg_info(data)
    coef, quant = o.jpeg_coefficients(data)
    return decode_reduced(coef, quant, info.width, info.height, info.components, info.h_samp, info.v_samp, info.orientation, d)
