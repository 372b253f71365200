"""A restatement of PNG decoding to the image cv2.imread(path, IMREAD_COLOR) returns, written from the PNG specification (sections 7, 9) and from the
transformations OpenCV's grfmt_png.cpp asks libpng for; not from csrc/.  zlib.decompress inflates; the unfilter is a plain loop over bytes.
tests/test_png_decode_ref.py pins it to Pillow.

  unfilter    Recon(x) = Filt(x) + predictor(a, b, c) mod 256; a = the byte bpp back (0 for the first bpp bytes), b = the byte above (0 on the first
              row), c = the byte above a; Avg = (a + b) >> 1 on the 9-bit sum; Paeth = the first of a, b, c nearest to a + b - c.
  samples     below 8 bits: packed MSB first; 16 bits: big-endian.
  expansion   png_set_strip_16: the high byte.  png_set_expand_gray_1_2_4_to_8: bit replication (x255, x85, x17).  png_set_palette_to_rgb: PLTE;
              an index past PLTE's end is a libpng error, so cv2 returns None.  png_set_strip_alpha: alpha dropped, never composited.
              png_set_gray_to_rgb, png_set_bgr: B = G = R = gray; R, G, B -> B, G, R.  tRNS, gAMA and the other ancillary chunks change nothing.
"""
import struct
import zlib

import numpy as np

import png_encode_ref as R

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def header(data):
    """dict of IHDR's fields, the palette (u8 [k, 3] or None) and the concatenated IDAT payload; every CRC is checked (png_encode_ref.parse)"""
    chunks = R.parse(data)
    assert chunks[0][0] == b"IHDR" and chunks[-1][0] == b"IEND"
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    pal = [b for k, b in chunks if k == b"PLTE"]
    return {"width": w, "height": h, "depth": depth, "type": ctype, "interlace": lace,
            "palette": np.frombuffer(pal[0], np.uint8).reshape(-1, 3) if pal else None, "idat": b"".join(b for k, b in chunks if k == b"IDAT")}


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def unfilter(filtered, height, row_bytes, bpp):
    """bytes of height * (1 + row_bytes) -> (u8 [height, row_bytes], the rows' filter bytes)"""
    assert len(filtered) == height * (1 + row_bytes)
    out = np.zeros((height, row_bytes), np.uint8)
    prev = bytearray(row_bytes)
    filters = []
    for r in range(height):
        f, line = filtered[r * (1 + row_bytes)], bytearray(filtered[r * (1 + row_bytes) + 1:(r + 1) * (1 + row_bytes)])
        filters.append(f)
        assert f <= 4
        if f == 1:
            for x in range(bpp, row_bytes):
                line[x] = (line[x] + line[x - bpp]) & 255
        elif f == 2:
            for x in range(row_bytes):
                line[x] = (line[x] + prev[x]) & 255
        elif f == 3:
            for x in range(row_bytes):
                line[x] = (line[x] + (((line[x - bpp] if x >= bpp else 0) + prev[x]) >> 1)) & 255
        elif f == 4:
            for x in range(row_bytes):
                a, c = (line[x - bpp], prev[x - bpp]) if x >= bpp else (0, 0)
                line[x] = (line[x] + paeth(a, prev[x], c)) & 255
        out[r] = np.frombuffer(bytes(line), np.uint8)
        prev = line
    return out, filters


def samples(rows, width, color_type, depth):
    """u8 [H, row_bytes] -> int [H, width, channels], the samples at their own depth"""
    H, ch = rows.shape[0], CHANNELS[color_type]
    if depth == 8:
        return rows[:, :width * ch].reshape(H, width, ch).astype(np.int64)
    if depth == 16:
        return np.ascontiguousarray(rows[:, :2 * width * ch]).view(">u2").reshape(H, width, ch).astype(np.int64)
    bits = np.unpackbits(rows, axis=1)[:, :width * depth].reshape(H, width, depth).astype(np.int64)
    return (bits << np.arange(depth - 1, -1, -1)).sum(axis=2).reshape(H, width, 1)


def expand(s, color_type, depth, palette):
    """samples -> (BGR u8 [H, W, 3], ok); ok False: a palette index past the palette's end (that pixel is black)"""
    H, W = s.shape[:2]
    if color_type == 3:
        k = len(palette)
        table = np.zeros((256, 3), np.uint8)
        table[:k] = palette
        rgb = table[s[:, :, 0]]
        return np.ascontiguousarray(rgb[:, :, ::-1]), bool((s[:, :, 0] < k).all())
    if depth == 16:
        s = s >> 8
    elif depth < 8:
        s = s * {1: 255, 2: 85, 4: 17}[depth]
    colour = s[:, :, :3] if color_type in (2, 6) else np.repeat(s[:, :, :1], 3, axis=2)
    return np.ascontiguousarray(colour[:, :, ::-1].astype(np.uint8)), True


def decode_samples(data):
    """(samples int [H, W, channels], header dict, the rows' filter bytes)"""
    h = header(data)
    assert h["interlace"] == 0
    ch = CHANNELS[h["type"]]
    row_bytes, bpp = (h["width"] * ch * h["depth"] + 7) // 8, max(1, ch * h["depth"] // 8)
    rows, filters = unfilter(zlib.decompress(h["idat"]), h["height"], row_bytes, bpp)
    return samples(rows, h["width"], h["type"], h["depth"]), h, filters


def decode(data):
    """the file as cv2.imread(path, IMREAD_COLOR) returns it: BGR u8 [H, W, 3], or None for an index past the palette's end"""
    s, h, _ = decode_samples(data)
    img, ok = expand(s, h["type"], h["depth"], h["palette"])
    return img if ok else None
