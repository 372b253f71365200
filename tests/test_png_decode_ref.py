"""CPU: pins the restatement the GPU PNG decoder is tested against (tests/png_decode_ref.py) and the file builder (tests/png_craft.py) to Pillow, on
crafted files of every colour type and bit depth under every filter, and on files Pillow writes.  Pillow keeps 16-bit gray as 16 bits (mode I;16)
where cv2's IMREAD_COLOR keeps the high byte, and its RGBA / LA / P modes still carry alpha or indices: there the SAMPLES are compared, before the
expansion, and the expansion rule is applied to both sides; everywhere else the finished BGR image is compared with Pillow's convert('RGB')."""
import io

import numpy as np
import pytest

import png_craft as K
import png_decode_ref as D

PIL = pytest.importorskip("PIL.Image")


def pillow_open(data):
    im = PIL.open(io.BytesIO(data))
    im.load()
    return im


@pytest.mark.parametrize("color_type,depth", K.ALL_FORMATS)
def test_crafted_files_decode_as_in_pillow(color_type, depth):
    for H, W, filters in ((5, 7, [0, 1, 2, 3, 4]), (9, 13, [4, 3, 2, 1, 0, 4, 4, 3, 3]), (3, 1, 4), (1, 9, 3), (6, 10, 1)):
        pal = K.random_palette(min(1 << depth, 200), seed=depth) if color_type == 3 else None
        s = K.random_samples(H, W, color_type, depth, seed=W, limit=len(pal) if pal is not None else None)
        data = K.make_png(s, color_type, depth, filters, palette=pal)
        got_s, h, got_f = D.decode_samples(data)
        assert (got_s == s).all() and got_f == list(np.broadcast_to(filters, (H,)))          # the craft's filters invert to the samples asked for
        im = pillow_open(data)
        assert im.size == (W, H)
        ours = D.decode(data)
        if color_type == 0 and depth == 16:
            assert (np.asarray(im).astype(np.int64) == s[:, :, 0]).all()                     # Pillow: the 16-bit samples themselves
            assert (ours[:, :, 0] == (s[:, :, 0] >> 8)).all() and (ours[:, :, 0] == ours[:, :, 1]).all() and (ours[:, :, 0] == ours[:, :, 2]).all()
        elif color_type == 3:
            assert (np.asarray(im) == s[:, :, 0]).all()                                      # the indices
            assert (np.asarray(im.convert("RGB"))[:, :, ::-1] == ours).all()
        elif color_type in (4, 6):
            a = np.asarray(im if color_type == 6 else im.convert("LA"))                      # LA / RGBA, 16-bit files by their high bytes (16-bit LA opens as RGBA)
            assert (a == (s >> (depth - 8))).all()
            colour = a[:, :, :3] if color_type == 6 else np.repeat(a[:, :, :1], 3, axis=2)
            assert (colour[:, :, ::-1] == ours).all()                                        # alpha dropped, the colour kept whatever the alpha
        else:
            assert (np.asarray(im.convert("RGB"))[:, :, ::-1] == ours).all()                 # 1-bit -> 0 / 255, 2- and 4-bit replicated, RGB16 high bytes


def test_pillow_written_files():
    rs = np.random.RandomState(5)
    H, W = 23, 31
    cases = {
        "L": PIL.fromarray(rs.randint(0, 256, (H, W), dtype=np.uint8)),
        "RGB": PIL.fromarray(rs.randint(0, 256, (H, W, 3), dtype=np.uint8)),
        "RGBA": PIL.fromarray(rs.randint(0, 256, (H, W, 4), dtype=np.uint8)),
        "LA": PIL.fromarray(rs.randint(0, 256, (H, W, 2), dtype=np.uint8), "LA"),
        "1": PIL.fromarray(rs.randint(0, 2, (H, W), dtype=np.uint8) * 255).convert("1"),
        "I;16": PIL.fromarray(rs.randint(0, 65536, (H, W)).astype(np.uint16)),
    }
    p = PIL.fromarray(rs.randint(0, 40, (H, W), dtype=np.uint8), "P")
    p.putpalette(K.random_palette(40).tobytes())
    cases["P"] = p
    for mode, im in cases.items():
        for kw in ({}, {"optimize": True}, {"compress_level": 0}):
            buf = io.BytesIO()
            im.save(buf, "PNG", **kw)
            ours = D.decode(buf.getvalue())
            if mode == "I;16":
                want = np.repeat((np.asarray(im).astype(np.int64) >> 8)[:, :, None], 3, axis=2)
            elif mode in ("RGBA", "LA"):
                a = np.asarray(im)
                want = (a[:, :, :3] if mode == "RGBA" else np.repeat(a[:, :, :1], 3, axis=2))[:, :, ::-1]
            else:
                want = np.asarray(im.convert("RGB"))[:, :, ::-1]
            assert ours.shape == (H, W, 3) and (ours == want).all(), (mode, kw)


def test_padding_bits_and_palette_end():
    """the ones in the padding bits of a partial last byte are not samples; an index at the palette's end is refused, the last one before it is not"""
    s = np.zeros((2, 3, 1), np.int64)
    data = K.make_png(s, 0, 1, [0, 2])
    assert (D.decode(data) == 0).all() and D.header(data)["idat"]
    pal = K.random_palette(3)
    ok = K.make_png(np.array([[[0], [1], [2]]]), 3, 2, 0, palette=pal)
    assert (D.decode(ok)[0] == pal[:, ::-1]).all()
    assert D.decode(K.make_png(np.array([[[0], [3], [2]]]), 3, 2, 0, palette=pal)) is None
    assert pillow_open(ok).size == (3, 1)


def test_ancillary_chunks_change_nothing():
    s = K.random_samples(4, 5, 2, 8)
    plain = K.make_png(s, 2, 8, 4)
    extra = K.make_png(s, 2, 8, 4, before_idat=[(b"gAMA", (45455).to_bytes(4, "big")), (b"tRNS", bytes(6))], after_idat=[(b"tEXt", b"k\0v")], split=[0, 3, 0, 1])
    assert (D.decode(plain) == D.decode(extra)).all() and (np.asarray(pillow_open(extra).convert("RGB")) == s).all()
