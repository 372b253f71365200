"""Builds PNG files for the decoder's tests from the DECODED samples: the caller chooses the image and every row's filter, so the neighbours that Sub,
Avg and Paeth see while unfiltering are under the test's control.  The forward filters are tests/png_encode_ref.py's (any bpp); the container, the
bit packing, the IDAT splitting and the zlib settings are here.  Nothing of the library under test is used."""
import struct
import zlib

import numpy as np

import png_encode_ref as R

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
ALL_FORMATS = [(t, d) for t in (0, 2, 3, 4, 6) for d in DEPTHS[t]]


def bpp_of(color_type, depth):
    return max(1, CHANNELS[color_type] * depth // 8)


def row_bytes_of(width, color_type, depth):
    return (width * CHANNELS[color_type] * depth + 7) // 8


def pack_rows(samples, color_type, depth, pad_ones=True):
    """samples int [H, W, channels] (or [H, W] for one channel), each below 2 ** depth -> u8 [H, row_bytes]: big-endian 16-bit samples, samples below
    8 bits packed MSB first; the padding bits of a partial last byte are ones unless pad_ones is False"""
    s = np.asarray(samples)
    if s.ndim == 2:
        s = s[:, :, None]
    H, W, ch = s.shape
    assert ch == CHANNELS[color_type] and depth in DEPTHS[color_type] and s.min() >= 0 and s.max() < (1 << depth)
    if depth == 8:
        return np.ascontiguousarray(s.reshape(H, W * ch).astype(np.uint8))
    if depth == 16:
        return np.ascontiguousarray(s.reshape(H, W * ch).astype(">u2")).view(np.uint8).reshape(H, 2 * W * ch)
    bits = ((s.reshape(H, W, 1).astype(np.uint8) >> np.arange(depth - 1, -1, -1, dtype=np.uint8)) & 1).reshape(H, W * depth)
    pad = -bits.shape[1] % 8
    bits = np.concatenate([bits, np.full((H, pad), 1 if pad_ones else 0, np.uint8)], axis=1)
    return np.packbits(bits, axis=1)


def filter_image(rows, bpp, filters):
    """u8 [H, row_bytes] unfiltered rows -> the filtered image's bytes, row r under filters[r] (0..4)"""
    H = rows.shape[0]
    filters = np.broadcast_to(np.asarray(filters, np.int64), (H,))
    f = R.filter_rows(rows, bpp).astype(np.uint8)
    out = np.empty((H, rows.shape[1] + 1), np.uint8)
    out[:, 0] = filters
    out[:, 1:] = f[filters, np.arange(H)]
    return out.tobytes()


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(data) + c.flush()


def split_idat(payload, split):
    """the IDAT chunks of a payload cut into pieces of the lengths in `split` (zeros allowed), the rest in a last one"""
    chunks, at = [], 0
    for n in split or []:
        chunks.append(R.chunk(b"IDAT", payload[at:at + n]))
        at += n
    chunks.append(R.chunk(b"IDAT", payload[at:]))
    return b"".join(chunks)


def assemble(width, height, color_type, depth, payload, palette=None, split=None, before_idat=(), after_idat=(), interlace=0):
    """a file around a finished zlib stream; palette u8 [k, 3] RGB; before_idat / after_idat: (type, body) chunks put there"""
    out = R.SIGNATURE + R.chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, color_type, 0, 0, interlace))
    if palette is not None:
        out += R.chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    for kind, body in before_idat:
        out += R.chunk(kind, body)
    out += split_idat(payload, split)
    for kind, body in after_idat:
        out += R.chunk(kind, body)
    return out + R.chunk(b"IEND", b"")


def make_png(samples, color_type, depth, filters=0, palette=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, split=None, before_idat=(), after_idat=(),
             pad_ones=True):
    """the file whose decoded samples are `samples`"""
    rows = pack_rows(samples, color_type, depth, pad_ones)
    s = np.asarray(samples)
    payload = deflate(filter_image(rows, bpp_of(color_type, depth), filters), level, strategy, wbits)
    return assemble(s.shape[1], s.shape[0], color_type, depth, payload, palette, split, before_idat, after_idat)


def random_samples(H, W, color_type, depth, seed=0, limit=None):
    """int [H, W, channels]; limit: an exclusive bound below 2 ** depth (palette indices)"""
    rs = np.random.RandomState(seed * 7919 + H * 131 + W * 17 + color_type * 5 + depth)
    return rs.randint(0, limit or (1 << depth), (H, W, CHANNELS[color_type]))


def random_palette(k, seed=0):
    return np.random.RandomState(1000 + seed + k).randint(0, 256, (k, 3)).astype(np.uint8)
