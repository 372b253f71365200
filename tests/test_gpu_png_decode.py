"""GPU: the PNG decoder (csrc/host_png.cpp + csrc/k19_png_decode.hip) through Context and imgcodecs against the restatement tests/png_decode_ref.py,
exact bytes.  The files come from tests/png_craft.py, which takes the DECODED image and every row's filter, so what Sub, Avg and Paeth see is
chosen here.  The images are tiny on purpose: the kernels go wrong at edges, not at size.

The kernels' tiling (csrc/k19_png_decode.hip): stripes of K_STRIPE rows and chunks of K_CHUNK bytes in k_png_segments, K_SCAN pixels per step and
K_ROWS rows per workgroup in k_png_rows, K_EXPAND pixels per workgroup in k_png_expand."""
import io
import os

import numpy as np
import pytest

import png_craft as K
import png_decode_ref as D

pytestmark = pytest.mark.gpu

K_STRIPE, K_CHUNK, K_SCAN, K_ROWS, K_EXPAND = 64, 512, 64, 4, 256
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    import sudoku_vision_amd as sva
    return sva.Context()


@pytest.fixture(scope="module")
def codecs():
    from sudoku_vision_amd import imgcodecs
    return imgcodecs


def check(codecs, ctx, data, what=""):
    want = D.decode(data)
    got = codecs.imdecode_png(data, ctx=ctx)
    assert want is not None and got is not None, what
    assert got.dtype == np.uint8 and got.shape == want.shape and (got == want).all(), what
    return got


def cycle(H, first=0):
    return [(first + r) % 5 for r in range(H)]


HEIGHTS = [1, 2, 63, 64, 65, 128, 129]
WIDTHS = [1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257]
GEOMETRY = sorted({(h, w) for i, h in enumerate(HEIGHTS) for w in (WIDTHS[i], WIDTHS[(i + 5) % 12], WIDTHS[(i + 9) % 12])} |
                  {(h, w) for i, w in enumerate(WIDTHS) for h in (HEIGHTS[i % 7], HEIGHTS[(i + 2) % 7], HEIGHTS[(i + 4) % 7])})


def test_geometry_covers_the_issue():
    for h in HEIGHTS:
        assert len({w for hh, w in GEOMETRY if hh == h}) >= 3
    for w in WIDTHS:
        assert len({h for h, ww in GEOMETRY if ww == w}) >= 3


@pytest.mark.parametrize("H,W", GEOMETRY)
def test_geometry_rgb_mixed_filters(codecs, ctx, H, W):
    s = K.random_samples(H, W, 2, 8, seed=1)
    for filters in (cycle(H), 4, 1):
        check(codecs, ctx, K.make_png(s, 2, 8, filters), (H, W, filters))


@pytest.mark.parametrize("row_bytes", [K_CHUNK - 1, K_CHUNK, K_CHUNK + 1, 2 * K_CHUNK, 2 * K_CHUNK + 1])
@pytest.mark.parametrize("H", [3, K_STRIPE + 1])
def test_chunk_edges(codecs, ctx, row_bytes, H):
    """rows of one below, at and one above a chunk of k_png_segments (gray, bpp 1), and RGB and 16-bit RGBA rows that straddle it (bpp 3, 8)"""
    s = K.random_samples(H, row_bytes, 0, 8, seed=2)
    for filters in (cycle(H, 3), 3, 4):
        check(codecs, ctx, K.make_png(s, 0, 8, filters), filters)
    check(codecs, ctx, K.make_png(K.random_samples(H, row_bytes // 3 + 1, 2, 8, seed=3), 2, 8, cycle(H, 4)))
    check(codecs, ctx, K.make_png(K.random_samples(H, row_bytes // 8 + 1, 6, 16, seed=4), 6, 16, cycle(H, 2)))


@pytest.mark.parametrize("W", [K_SCAN - 1, K_SCAN, K_SCAN + 1, K_EXPAND - 1, K_EXPAND, K_EXPAND + 1, 2 * K_EXPAND + 1])
def test_row_scan_edges(codecs, ctx, W):
    """all-Sub and all-None files (every row its own segment) around the prefix sum's step and the expansion's workgroup, H around K_ROWS"""
    for H in (K_ROWS - 1, K_ROWS, K_ROWS + 1):
        for color_type, depth in ((2, 8), (0, 8), (6, 16), (4, 8)):
            s = K.random_samples(H, W, color_type, depth, seed=5)
            check(codecs, ctx, K.make_png(s, color_type, depth, 1))
            check(codecs, ctx, K.make_png(s, color_type, depth, 0))


@pytest.mark.parametrize("color_type,depth", K.ALL_FORMATS)
def test_every_format(codecs, ctx, color_type, depth):
    """every (colour type, depth): bpp 1, 2, 3, 4, 6, 8 and packed rows whose last byte is partial, its padding bits ones"""
    for H, W in ((5, 7), (66, 13), (9, 67)):
        pal = K.random_palette(1 << depth, seed=depth) if color_type == 3 else None
        s = K.random_samples(H, W, color_type, depth, seed=6)
        if depth < 8:
            assert (W * depth) % 8                                      # a partial last byte
        for filters in (cycle(H), cycle(H, 4), 1, 0):
            check(codecs, ctx, K.make_png(s, color_type, depth, filters, palette=pal, pad_ones=True), (H, W, filters))


@pytest.mark.parametrize("f", [0, 1, 2, 3, 4])
def test_each_filter_everywhere_and_first(codecs, ctx, f):
    for color_type, depth in ((2, 8), (0, 8), (6, 8), (0, 16)):
        s = K.random_samples(70, 33, color_type, depth, seed=7 + f)
        check(codecs, ctx, K.make_png(s, color_type, depth, f))                              # on every row
        for rest in (0, 1, 2, 3, 4):
            check(codecs, ctx, K.make_png(s, color_type, depth, [f] + [rest] * 69))           # on the first row only


def test_segment_lengths(codecs, ctx):
    """segments of 1, 2, 64 and 65 rows, the restart rows (None or Sub) placed accordingly; then all-Paeth over 129 rows: one segment, three stripes"""
    filters = []
    for k, n in enumerate((1, 2, K_STRIPE, K_STRIPE + 1, 1, 1, 2)):
        filters += [k % 2] + [2 + (r + k) % 3 for r in range(n - 1)]
    H = len(filters)
    for color_type, depth, W in ((2, 8, 40), (0, 8, 600), (0, 1, 35)):
        s = K.random_samples(H, W, color_type, depth, seed=8)
        check(codecs, ctx, K.make_png(s, color_type, depth, filters))
    for f in (4, 3, 2):
        check(codecs, ctx, K.make_png(K.random_samples(2 * K_STRIPE + 1, 200, 2, 8, seed=9), 2, 8, f))
    check(codecs, ctx, K.make_png(K.random_samples(2 * K_STRIPE + 1, 50, 2, 8, seed=9), 2, 8, [1] + [4] * (2 * K_STRIPE)))


def test_paeth_triples(codecs, ctx):
    """(a, b, c) through every triple of {0, 1, 2, 127, 128, 129, 253, 254, 255}^3: a gray image whose row 2t holds c, b and row 2t + 1 holds a, x at
    columns 2j, 2j + 1, so the Paeth row's pixel 2j + 1 sees left a, above b, above-left c: every tie, and p - a, p - b, p - c of both signs and 0"""
    vals = [0, 1, 2, 127, 128, 129, 253, 254, 255]
    triples = [(a, b, c) for a in vals for b in vals for c in vals]
    per_row = 32
    rows = -(-len(triples) // per_row)
    img = np.zeros((2 * rows, 2 * per_row), np.int64)
    for k, (a, b, c) in enumerate(triples):
        r, j = divmod(k, per_row)
        img[2 * r, 2 * j], img[2 * r, 2 * j + 1] = c, b
        img[2 * r + 1, 2 * j], img[2 * r + 1, 2 * j + 1] = a, (a * 7 + b * 3 + c + k) % 256
    assert img.shape[0] <= 64 and img.shape[1] == 64
    filters = [0, 4] * rows
    check(codecs, ctx, K.make_png(img[:, :, None], 0, 8, filters))
    check(codecs, ctx, K.make_png(img[:, :, None], 0, 8, [1] + [4] * (2 * rows - 1)))
    check(codecs, ctx, K.make_png(np.repeat(img[:, :, None], 3, axis=2) ^ np.array([0, 1, 255]), 2, 8, 4))


def test_avg_sub_up_wrap(codecs, ctx):
    img = np.full((6, 40, 1), 255, np.int64)
    check(codecs, ctx, K.make_png(img, 0, 8, 3))                                              # Avg with a = b = 255: the 9-bit sum
    img[::2, ::2] = 254                                                                      # a + b odd
    img[1::2, 1::3] = 0
    for f in (3, 1, 2, [1, 2, 3, 3, 2, 1]):
        check(codecs, ctx, K.make_png(img, 0, 8, f))
    ramp = (np.arange(6 * 40).reshape(6, 40, 1) * 97) % 256                                   # Sub and Up sums that wrap past 255 again and again
    for f in (1, 2):
        check(codecs, ctx, K.make_png(ramp, 0, 8, f))
        check(codecs, ctx, K.make_png(np.repeat(ramp, 4, axis=2), 6, 8, f))


@pytest.mark.parametrize("entries", [1, 2, 16, 256])
def test_palettes(codecs, ctx, entries):
    depth = 8 if entries > 16 else 4 if entries > 2 else 1
    pal = K.random_palette(entries)
    s = K.random_samples(9, 21, 3, depth, seed=10, limit=entries)
    got = check(codecs, ctx, K.make_png(s, 3, depth, cycle(9), palette=pal))
    assert (got == pal[s[:, :, 0]][:, :, ::-1]).all()
    if entries < (1 << depth):
        s[4, 5, 0] = entries                                            # the first index past the end
        data = K.make_png(s, 3, depth, cycle(9), palette=pal)
        assert D.decode(data) is None and codecs.imdecode_png(data, ctx=ctx) is None
        s[4, 5, 0] = entries - 1
        check(codecs, ctx, K.make_png(s, 3, depth, cycle(9), palette=pal))                    # and the context decodes the next file


def test_sixteen_bit_alpha_and_ancillary(codecs, ctx):
    s = np.zeros((4, 6, 3), np.int64)
    s[:, ::2] = 0x00FF                                                                       # low byte ff, high byte 00 -> 0
    s[:, 1::2] = 0xFF00                                                                      # and the reverse -> 255
    got = check(codecs, ctx, K.make_png(s, 2, 16, [0, 1, 3, 4]))
    assert (got[:, ::2] == 0).all() and (got[:, 1::2] == 255).all()
    g = np.zeros((4, 6, 1), np.int64)
    g[:, ::2], g[:, 1::2] = 0x00FF, 0xFF00
    got = check(codecs, ctx, K.make_png(g, 0, 16, 2))
    assert (got[:, ::2] == 0).all() and (got[:, 1::2] == 255).all()
    rgba = K.random_samples(5, 9, 6, 8, seed=11)
    rgba[:, :, :3] |= 1
    rgba[:, :, 3] = 0                                                                        # alpha 0 over a non-zero colour: the colour is kept
    got = check(codecs, ctx, K.make_png(rgba, 6, 8, cycle(5)))
    assert (got == rgba[:, :, 2::-1]).all()
    la = K.random_samples(5, 9, 4, 16, seed=12)
    la[:, :, 1] = 0
    got = check(codecs, ctx, K.make_png(la, 4, 16, cycle(5)))
    assert (got[:, :, 0] == la[:, :, 0] >> 8).all()
    rgb = K.random_samples(5, 9, 2, 8, seed=13)
    extra = K.make_png(rgb, 2, 8, cycle(5), before_idat=[(b"gAMA", (45455).to_bytes(4, "big")), (b"tRNS", bytes([0, 1, 0, 2, 0, 3]))], after_idat=[(b"tEXt", b"a\0b")],
                       split=[0, 1, 2, 0, 3])
    got = check(codecs, ctx, extra)
    assert (got == rgb[:, :, ::-1]).all()
    for level, strategy in ((0, 0), (9, 0), (1, 3), (6, 4)):                                  # stored, dynamic, RLE and fixed blocks end to end
        check(codecs, ctx, K.make_png(rgb, 2, 8, 4, level=level, strategy=strategy, wbits=9 if level else 15))


def test_pitch_stride_batch_and_repeat(codecs, ctx):
    import torch
    H, W = 37, 29
    files = [K.make_png(K.random_samples(H, W, 2, 8, seed=20 + i), 2, 8, cycle(H, i)) for i in range(3)]
    want = [D.decode(f) for f in files]
    singles = [ctx.imdecode_png(f) for f in files]
    batch = ctx.imdecode_png_batch(files, threads=2)
    assert batch.is_cuda and tuple(batch.shape) == (3, H, W, 3)
    for i in range(3):
        assert (singles[i].cpu().numpy() == want[i]).all() and (batch[i].cpu().numpy() == want[i]).all()
    assert (ctx.imdecode_png(files[1]).cpu().numpy() == want[1]).all()                       # the same file again
    # an output with row padding and a gap between frames: the padding and the gap keep their bytes
    big = torch.full((3, H + 2, W + 5, 3), 0xA5, dtype=torch.uint8, device=ctx.device)
    view = big[:, :H, :W]
    ctx.imdecode_png_batch(files, threads=1, out=view)
    host = big.cpu().numpy()
    for i in range(3):
        assert (host[i, :H, :W] == want[i]).all()
    assert (host[:, H:] == 0xA5).all() and (host[:, :, W:] == 0xA5).all()
    other = K.make_png(K.random_samples(H, W + 1, 2, 8), 2, 8, 0)
    with pytest.raises(ValueError):
        ctx.imdecode_png_batch([files[0], other])
    with pytest.raises(ValueError):
        ctx.imdecode_png_batch([files[0], K.make_png(K.random_samples(H, W, 6, 8), 6, 8, 0)])


def test_device_tensor_feeds_the_pipeline(codecs, ctx, tmp_path):
    """device=True: a CUDA tensor that recognize_image takes as it is, with the result of the same frame decoded from its JPEG"""
    import torch
    import cnn_oracle
    from PIL import Image
    from sudoku_vision_amd.pipeline import recognize_image
    frame = codecs.imread(os.path.join(GOLDEN, "sample_2.jpg"), ctx=ctx)
    assert frame is not None
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(buf, "PNG", compress_level=1)
    path = tmp_path / "frame.png"
    path.write_bytes(buf.getvalue())
    dev = codecs.imread_png(path, device=True, ctx=ctx)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and (dev.cpu().numpy() == frame).all()
    g2 = np.load(os.path.join(GOLDEN, "cnn_coreml_fp16.npz"))
    ctx.load_state_dict({k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS})
    a, b = recognize_image(frame, ctx=ctx), recognize_image(dev, ctx=ctx)
    assert (a is None) == (b is None)
    if a is not None:
        assert (a["digits"] == b["digits"]).all() and (a["corners"] == b["corners"]).all()


def test_refusals(codecs, ctx, tmp_path):
    from sudoku_vision_amd._native import NativeError
    s = K.random_samples(8, 8, 2, 8)
    good = K.make_png(s, 2, 8, 4)
    rows = K.pack_rows(s, 2, 8)
    adam7 = K.assemble(8, 8, 2, 8, K.deflate(K.filter_image(rows, 3, 0)), interlace=1)
    with pytest.raises(NativeError, match="UNSUPPORTED"):
        codecs.imdecode_png(adam7, ctx=ctx)
    assert codecs.imdecode_png(good[:len(good) // 2], ctx=ctx) is None
    assert codecs.imdecode_png(good[:-1], ctx=ctx) is None
    assert codecs.imdecode_png(b"not a png", ctx=ctx) is None
    assert codecs.imread_png(tmp_path / "missing.png", ctx=ctx) is None
    assert codecs.imread_png(tmp_path, ctx=ctx) is None
    check(codecs, ctx, good)


@pytest.mark.parametrize("params", [None, [16, 6], [16, 0]])
def test_round_trip_with_the_encoder(codecs, ctx, params):
    """imdecode_png(imencode_png(img)) == img with the encoder's defaults (all Sub), adaptive rows (compression 6) and stored blocks (compression 0)"""
    rs = np.random.RandomState(31)
    y, x = np.mgrid[0:90, 0:130]
    smooth = ((x * 2 + y * 3) % 256).astype(np.uint8)
    bgr = np.stack([smooth, 255 - smooth, rs.randint(0, 256, smooth.shape).astype(np.uint8)], axis=2)
    for img in (bgr, smooth, np.array([[[7, 200, 31]]], np.uint8), np.array([[9]], np.uint8)):
        ok, data = codecs.imencode_png(img, params, ctx=ctx)
        assert ok
        got = codecs.imdecode_png(data, ctx=ctx)
        want = img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2)
        assert got is not None and got.shape == want.shape and (got == want).all()
        assert (D.decode(data.tobytes()) == want).all()


def test_real_frame(codecs, ctx):
    """tests/golden/sample_2.jpg cropped to 320 x 240: written by Pillow (its adaptive filters) and by png_craft as all-Paeth"""
    from PIL import Image
    frame = codecs.imread(os.path.join(GOLDEN, "sample_2.jpg"), ctx=ctx)
    assert frame is not None and frame.shape[0] >= 240 and frame.shape[1] >= 320
    crop = np.ascontiguousarray(frame[:240, :320])
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(crop[:, :, ::-1])).save(buf, "PNG")
    got = codecs.imdecode_png(buf.getvalue(), ctx=ctx)
    assert (got == crop).all()
    filters = D.decode_samples(buf.getvalue())[2]
    assert len(set(filters)) > 1                                        # Pillow did choose per row
    got = codecs.imdecode_png(K.make_png(crop[:, :, ::-1].astype(np.int64), 2, 8, 4), ctx=ctx)
    assert (got == crop).all()
