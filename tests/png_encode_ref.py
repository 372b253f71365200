"""A numpy restatement of what the PNG encoder puts INTO its deflate stream: the filtered bytes (PNG specification, section 9: filter-type byte, then
the row filtered from the original left / above / above-left neighbours; the first row's "above" is zero; left neighbours are bpp bytes back), for
the five fixed filters and for `adaptive` -- per row the filter whose output has the smallest sum of abs((int8) byte), the lowest filter number on a
tie (libpng's default heuristic).  Written from the specification, not from csrc/sv_png_band.h.  tests/test_png_encode_ref.py pins it to Pillow: a
file made of these bytes decodes to the input.  zlib_rle is the size reference: zlib at cv2's defaults (level 1, Z_RLE).

Also the container's parser used by the tests: chunks with verified CRCs."""
import struct
import zlib

import numpy as np

FILTERS = ["none", "sub", "up", "average", "paeth", "adaptive"]
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def rgb_rows(img):
    """u8 [H,W,3] BGR or [H,W] gray -> (u8 [H, W * bpp] in file order, bpp)"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    if img.ndim == 2:
        return np.ascontiguousarray(img), 1
    assert img.shape[2] == 3
    return np.ascontiguousarray(img[:, :, ::-1]).reshape(img.shape[0], -1), 3


def filter_rows(rows, bpp):
    """int [5, H, rowbytes]: every row under every fixed filter"""
    x = rows.astype(np.int32)
    H, n = x.shape
    a = np.zeros_like(x); a[:, bpp:] = x[:, :-bpp] if n > bpp else 0
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, bpp:] = x[:-1, :-bpp] if n > bpp else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) & 255


def row_filters(img, mode):
    """the filter number of every row"""
    rows, bpp = rgb_rows(img)
    if mode != "adaptive":
        return np.full(rows.shape[0], FILTERS.index(mode), np.int64)
    f = filter_rows(rows, bpp).astype(np.uint8).view(np.int8).astype(np.int64)
    return np.argmin(np.abs(f).sum(axis=2), axis=0)                    # argmin: the first (lowest) on a tie


def filtered(img, mode="sub"):
    """bytes: the filtered image, H * (1 + W * bpp)"""
    rows, bpp = rgb_rows(img)
    f = filter_rows(rows, bpp).astype(np.uint8)
    which = row_filters(img, mode)
    out = np.empty((rows.shape[0], rows.shape[1] + 1), np.uint8)
    out[:, 0] = which
    out[:, 1:] = f[which, np.arange(rows.shape[0])]
    return out.tobytes()


def zlib_rle(data):
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return c.compress(data) + c.flush()


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def make_file(img, idat):
    """a PNG file around a finished zlib stream"""
    img = np.asarray(img)
    ihdr = struct.pack(">IIBBBBB", img.shape[1], img.shape[0], 8, 2 if img.ndim == 3 else 0, 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")


def parse(data):
    """[(kind, body)] of a file; asserts the signature, the framing and every CRC"""
    data = bytes(data)
    assert data[:8] == SIGNATURE
    at, chunks = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        assert len(body) == n and at + 12 + n <= len(data), "truncated chunk"
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), kind
        chunks.append((kind, body))
        at += 12 + n
    return chunks


def check_file(data, img):
    """The layout every file of this encoder has: IHDR, one IDAT, IEND; 8-bit, colour type 2 or 0, no interlace; the IDAT a zlib stream that
    starts 78 01.  Returns zlib.decompress(IDAT) (which verifies the Adler-32)."""
    img = np.asarray(img)
    chunks = parse(data)
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", img.shape[1], img.shape[0], 8, 2 if img.ndim == 3 else 0, 0, 0, 0)
    assert chunks[2][1] == b"" and chunks[1][1][:2] == b"\x78\x01"
    return zlib.decompress(chunks[1][1])


def pillow_decode(data):
    """the file's pixels in this library's convention (BGR or gray), and (mode, size)"""
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(data)))
    im.load()
    a = np.asarray(im)
    return (a if im.mode == "L" else np.ascontiguousarray(a[..., ::-1])), im.mode, im.size


def content(kind, H, W, gray=False):
    """test inputs: u8 [H,W,3] BGR, or [H,W] when gray"""
    shape = (H, W) if gray else (H, W, 3)
    rs = np.random.RandomState(H * 1000 + W + gray)
    if kind == "noise":
        return rs.randint(0, 256, shape, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(shape, np.uint8)
    if kind == "flat":
        return np.full(shape, 77, np.uint8) if gray else np.broadcast_to(np.array([10, 200, 77], np.uint8), shape).copy()
    if kind == "synthetic":
        # flat patches, ramps, a little noise and hard edges: every filter wins some row
        y, x = np.mgrid[0:H, 0:W]
        a = ((x // 9) * 37 + (y // 7) * 11) % 256
        a = np.where((x + y) % 23 < 11, a, (3 * x + 5 * y) % 256)
        a = np.where(y % 16 == 5, rs.randint(0, 256, (H, W)), a).astype(np.uint8)
        return a if gray else np.stack([a, (a.astype(np.int32) * 3 + x) % 256, 255 - a], 2).astype(np.uint8)
    raise ValueError(kind)


def photo_1080p(name):
    """a 1080 x 1920 BGR crop of a golden photo (tiled when the photo is smaller)"""
    import os
    from PIL import Image
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)
    rgb = np.asarray(Image.open(path).convert("RGB"))
    reps = (-(-1080 // rgb.shape[0]), -(-1920 // rgb.shape[1]), 1)
    rgb = np.tile(rgb, reps)
    y0, x0 = (rgb.shape[0] - 1080) // 2, (rgb.shape[1] - 1920) // 2
    return np.ascontiguousarray(rgb[y0:y0 + 1080, x0:x0 + 1920, ::-1])
